"""dgp_prior_samples on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through the planner.

  * supplied noise: th bit for bit against tests/prior_oracle.py, which restates the header's operation order, and info exactly -- n in {2, 3, 17, 64, 65, 130, 257}
    (ragged groups, the three lanes-per-trajectory instantiations and the block loop, each asserted to be reached from dgp_prior_launch_shape, the function the
    library's dispatch reads), B in {1, 5}, S in {1, 3, 7}, dof 2 and 3, fp64 and fp32 I/O, mean NULL and given, diagonal and full Q_c_inv, scale 0 / 0.3 / 1; scale 0
    returns the mean.  Not the full cross product: every n runs all 12 (mean, Q_c_inv, scale) combinations, each at ONE (B, S) pair, rotated with the combination and
    with n -- every pair occurs twice per n and with every n, but a given (n, combination) always meets the same pair (run time: 84 launches per dof and I/O type);
  * generated noise: the normals within 1e-13 of the oracle's (r <= 8.6 since 1 - u0 >= 2^-53, library errors <= 2 ulp, the angle rounded to 2 pi 2^-53: below
    1e-14, ten times that allowed), and feeding them back as noise reproduces th bit for bit;
  * purity: a problem alone and inside a batch, two batch positions with first_problem shifted, two runs, unaligned buffers, guard bands with every optional
    pointer NULL: the same bits;
  * mean NULL, scale 0 against th + dtheta of dgp_gn_step on an obstacle-free grid with reg = 0, at parity_cases.TOL;
  * capture / replay in a HIP graph, the timed launch, and the motivating multi-start case through the planner."""
import numpy as np
import pytest
import torch

import harness
import interp_oracle as IO_
import parity_cases as PC
import prior_cases as PC_
import prior_oracle as PO
from conftest import rel_err
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NS, PAIRS = (2, 3, 17, 64, 65, 130, 257), tuple((B, S) for B in (1, 5) for S in (1, 3, 7))
COMBOS = tuple((with_mean, qc, scale) for with_mean in (False, True) for qc in ('diag', 'full') for scale in (0.0, 0.3, 1.0))


@pytest.fixture(scope='module')
def be():
  return harness.Backend('hip')


def run(be, p, start, goal, S, mean=None, scale=1.0, noise=None, seed=0, first_problem=0, io='f64', want_noise=False, want_info=True):
  """dgp_prior_samples -> (th (B,S,n,d), noise_out (B,S,n+1,d) or None, info (B,S) or None) as numpy arrays"""
  be._keep, be._rec = [], {}
  solver = _capi.Solver(harness.config_from_oracle(p, io), api=be.api)
  B, n, d = start.shape[0], p.n, p.state_dim
  _, st_p = be.to_dev(start, io, name='start')
  _, go_p = be.to_dev(goal, io, name='goal')
  _, mn_p = be.to_dev(mean, io, name='mean')
  _, nz_p = be.to_dev(noise, dtype=np.float64, name='noise')
  th, th_p = be.empty((B, S, n, d), io, name='th')
  no, no_p = be.empty((B, S, n + 1, d), dtype=np.float64, name='noise_out') if want_noise else (None, None)
  info, info_p = be.empty((B, S), dtype=np.int32, name='info') if want_info else (None, None)
  solver.prior_samples(B, S, st_p, go_p, th_p, mn_p, scale, seed, first_problem, nz_p, no_p, info_p, be.stream())
  res = be.to_np(th), be.to_np(no), be.to_np(info)
  be._done()
  return res


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('dof', [2, 3])
def test_supplied_noise_bit_for_bit(be, dof, io):
  bad, shapes, flags = [], set(), set()
  for i, n in enumerate(NS):
    lanes, blocks = _capi.Solver(harness.config_from_oracle(PC_.params(dof, n), io), api=be.api).prior_launch_shape()      # what the library's own dispatch reads
    assert (lanes, blocks > 1) == (PO.lpt(n), PO.is_long(n)) and blocks == (n + 63) // 64, (n, lanes, blocks)
    shapes.add(('long', lanes) if blocks > 1 else ('short', lanes))
    for c, (with_mean, qc, scale) in enumerate(COMBOS):
      B, S = PAIRS[(c + i) % len(PAIRS)]
      p = PC_.params(dof, n, qc, K_s=0.05, K_g=0.02)
      start, goal, mean, z = PC_.inputs(dof, n, B, S, 100 * n + c, io, with_mean)
      want, winfo = PO.run(p, start, goal, z, mean, scale, io)
      got, _, info = run(be, p, start, goal, S, mean, scale, z, io=io)
      tag = 'dof %d %s n %d B %d S %d mean %s Q_c_inv %s scale %g' % (dof, io, n, B, S, with_mean, qc, scale)
      if not PC_.same_bits(got, want):
        k = tuple(np.argwhere(PC_.bits(got) != PC_.bits(want))[0])
        bad.append('%s: th differs from the oracle at %s: %r against %r' % (tag, k, got[k], want[k]))
      if not np.array_equal(info, winfo): bad.append('%s: info %s, expected %s' % (tag, info.ravel(), winfo.ravel()))
      if scale == 0.0:
        m = mean if with_mean else PO.mu(p, start, goal, io)
        if not np.array_equal(got, np.broadcast_to(m[:, None], got.shape)): bad.append('%s: scale 0 does not return the mean' % tag)
      flags |= set(winfo.ravel().tolist())
  assert shapes == {('short', 16), ('short', 32), ('short', 64), ('long', 64)}
  assert flags == {0, 1}      # samples inside the limits and samples that leave them (neither clamped nor rejected)
  assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_info_bits_are_exact(be, io):
  for dof, n in ((2, 17), (3, 130)):
    p = PC_.params(dof, n, 'full', K_s=0.05, K_g=0.02)
    start, goal, _, z = PC_.inputs(dof, n, 3, 4, 9, io, False)
    z[0, 1, 5, 1] = np.nan                      # one sample with a non-finite value: bit 1 (and bit 0: a NaN position is outside)
    z[2, 3, n, 0] = np.inf                      # ... through the goal observation
    z[1, 2] *= 0.0                              # the mean itself: inside
    start[1, 0, :dof], goal[1, 0, :dof] = 1.0, -2.0
    want, winfo = PO.run(p, start, goal, z, None, 1.0, io)
    got, _, info = run(be, p, start, goal, 4, None, 1.0, z, io=io)
    assert PC_.same_bits(got, want) and np.array_equal(info, winfo), (dof, n, info, winfo)
    assert info[0, 1] == 3 and info[2, 3] == 3 and info[1, 2] == 0
    # trajectories that leave the limits by far, without a NaN: bit 0 alone
    wide = PC_.inputs(dof, n, 3, 4, 10, io, False)[3]
    got, _, info = run(be, p, start, goal, 4, None, 40.0, wide, io=io)
    assert np.array_equal(info, PO.run(p, start, goal, wide, None, 40.0, io)[1]) and (info == 1).all() and np.isfinite(got).all()
    # without info the same th
    assert PC_.same_bits(run(be, p, start, goal, 4, None, 1.0, z, io=io, want_info=False)[0], want)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_generated_noise(be, io):
  for dof, n, B, S, seed, first in ((2, 17, 5, 3, 0, 0), (3, 64, 2, 7, (1 << 63) + 12345, (1 << 32) - 1), (2, 130, 3, 2, 7, 1 << 40), (3, 3, 5, 1, 1, 5)):
    p = PC_.params(dof, n, 'full', K_s=0.05, K_g=0.02)
    start, goal, mean, _ = PC_.inputs(dof, n, B, S, n, io)
    th, z, info = run(be, p, start, goal, S, mean, 0.5, None, seed, first, io, want_noise=True)
    want = PO.all_normals(seed, first, B, S, n, 2 * dof)
    assert z.shape == want.shape and np.isfinite(z).all() and np.abs(z - want).max() <= 1e-13, (dof, n, np.abs(z - want).max())
    # the normals fed back reproduce th bit for bit, and noise_out is then a copy; the oracle fed the same normals agrees as well
    th2, z2, info2 = run(be, p, start, goal, S, mean, 0.5, z, 99, 3, io, want_noise=True)
    assert PC_.same_bits(th2, th) and PC_.same_bits(z2, z) and np.array_equal(info2, info)
    assert PC_.same_bits(th, PO.run(p, start, goal, z, mean, 0.5, io)[0])
    # without noise_out the same th; another seed other samples
    assert PC_.same_bits(run(be, p, start, goal, S, mean, 0.5, None, seed, first, io)[0], th)
    assert not PC_.same_bits(run(be, p, start, goal, S, mean, 0.5, None, seed + 1, first, io)[0], th)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_purity(be, io):
  for dof, n, B, S in ((2, 17, 5, 3), (3, 64, 5, 7), (2, 130, 5, 2), (3, 2, 5, 3)):
    p = PC_.params(dof, n, 'full', K_s=0.05, K_g=0.02)
    start, goal, mean, _ = PC_.inputs(dof, n, B, S, 3 * n, io)
    for m in (None, mean):
      sub = lambda a, sl: None if a is None else a[sl]
      ref = run(be, p, start, goal, S, m, 0.7, None, 5, 10, io, want_noise=True)
      again = run(be, p, start, goal, S, m, 0.7, None, 5, 10, io, want_noise=True)
      assert all(PC_.same_bits(a, b) for a, b in zip(again, ref)), (dof, n, 'two runs')
      alone = run(be, p, start[2:3], goal[2:3], S, sub(m, slice(2, 3)), 0.7, None, 5, 12, io, want_noise=True)
      assert all(PC_.same_bits(a, b[2:3]) for a, b in zip(alone, ref)), (dof, n, 'alone')
      moved = run(be, p, start[1:], goal[1:], S, sub(m, slice(1, None)), 0.7, None, 5, 11, io, want_noise=True)
      assert all(PC_.same_bits(a, b[1:]) for a, b in zip(moved, ref)), (dof, n, 'batch position')
      fewer = run(be, p, start, goal, 1, m, 0.7, None, 5, 10, io)      # sample s does not depend on how many samples are drawn
      assert PC_.same_bits(fewer[0], ref[0][:, :1]), (dof, n, 'fewer samples')
      be.misalign = True      # every buffer one element past a 16-byte boundary: the element-wise stores
      try: mis = run(be, p, start, goal, S, m, 0.7, None, 5, 10, io, want_noise=True)
      finally: be.misalign = False
      assert all(PC_.same_bits(a, b) for a, b in zip(mis, ref)), (dof, n, 'unaligned')


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_guard_bands_with_the_optional_pointers_null(io):
  g = harness.Backend('hip')
  g.guard = True
  for mis in (False, True):
    g.misalign = mis
    for dof, n, B, S in ((2, 3, 5, 3), (3, 17, 3, 7), (2, 64, 5, 1), (3, 65, 2, 3), (2, 257, 1, 3)):
      p = PC_.params(dof, n, 'full', K_s=0.05, K_g=0.02)
      start, goal, _, z = PC_.inputs(dof, n, B, S, n, io, False)
      th = run(g, p, start, goal, S, None, 1.0, None, 3, 0, io, want_info=False)[0]      # mean, noise, noise_out and info NULL
      assert np.isfinite(th).all()
      full = run(g, p, start, goal, S, None, 1.0, None, 3, 0, io, want_noise=True)
      assert PC_.same_bits(full[0], th)
      assert PC_.same_bits(run(g, p, start, goal, S, None, 1.0, z, io=io, want_info=False)[0], PO.run(p, start, goal, z, None, 1.0, io)[0])
  assert g.guard_checks > 0 and g.input_checks > 0 and g.calls == 30


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_mean_is_one_obstacle_free_step_of_the_solver(be, io):
  """mean NULL, scale 0: th = th_0 + dtheta of dgp_gn_step from any th_0 on a grid far from every obstacle, with reg = 0 -- the tolerance of the parity cases"""
  for dof, n, qc in ((2, 17, 'diag'), (3, 17, 'full'), (2, 64, 'full'), (3, 65, 'diag')):
    p = PC_.params(dof, n, qc, reg=0.0)
    B = 3
    start, goal, th0, z = PC_.inputs(dof, n, B, 1, n + dof, io)
    sdf = np.full((1, 1, 16, 16), 50.0)
    dth, _, _, info = be.step(p, th0, start, goal, sdf, io=io)
    assert (info == 0).all()
    got = run(be, p, start, goal, 1, None, 0.0, z, io=io)[0][:, 0]
    want = th0 + dth
    assert rel_err(got, want) < PC.TOL[io], (dof, n, qc, rel_err(got, want))
    assert PC_.same_bits(got, PO.mu(p, start, goal, io))


def test_timed_launch(be):
  p = PC_.params(2, 64)
  start, goal, _, _ = PC_.inputs(2, 64, 5, 3, 1, 'f32', False)
  timer = _capi.KernelTimer(1, api=be.api)
  timer.arm()
  run(be, p, start, goal, 3, io='f32')
  torch.cuda.synchronize()
  ms = timer.durations_ms()
  assert len(ms) == 1 and 0.0 < ms[0] < 100.0, ms


def _planner(n, B=1, max_iters=10):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': max_iters, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)


def test_sample_prior_capture_and_replay():
  n, B, S = 17, 5, 3
  p = PC_.params(2, n, K_s=0.01, K_g=0.01)
  start, goal, mean, _ = PC_.inputs(2, n, B, S, 4)
  other = PC_.inputs(2, n, B, S, 5)[0]
  planner = _planner(n, B)
  st, go, mn, ot = (torch.from_numpy(a).to(DEV) for a in (start, goal, mean, other))
  call = lambda s: planner.sample_prior(s, go, S, seed=3, first_problem=7, scale=0.5, return_noise=True)
  outs = lambda r: (r[0], r[1].flags, r[1].noise)
  with torch.no_grad():
    eager, eager2 = call(st), call(ot)
    static_in = st.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      call(static_in)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out = call(static_in)
    for t in outs(out): t.fill_(-3)      # the replay, not the capture, must produce the values
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs(out), outs(eager)))
    static_in.copy_(ot)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs(out), outs(eager2))) and not torch.equal(eager[0], eager2[0])
  z = eager[1].noise.cpu().numpy()
  assert np.abs(z - PO.all_normals(3, 7, B, S, n, 4)).max() <= 1e-13
  assert PC_.same_bits(eager[0].cpu().numpy(), PO.run(p, start, goal, z, None, 0.5)[0])
  # around a given mean
  thm = planner.sample_prior(st, go, S, mean=mn, scale=0.25, noise=eager[1].noise)[0]
  assert PC_.same_bits(thm.cpu().numpy(), PO.run(p, start, goal, z, mean, 0.25)[0])
  # float32, supplied noise
  th32, info = planner.sample_prior(st.float(), go.float(), S, seed=3, first_problem=7, noise=eager[1].noise)
  assert th32.dtype == torch.float32 and info.noise is None
  assert PC_.same_bits(th32.cpu().numpy(), PO.run(p, PO.rnd(start, 'f32'), PO.rnd(goal, 'f32'), z, None, 1.0, 'f32')[0])


def test_motivating_case_through_the_planner():
  """one disc on the start-goal segment: forward() from the straight line ends in collision; of 16 samples of the prior several end collision-free with a finite
  error -- the outcome tests/prior_cases.py records from the CPU oracle's Gauss-Newton loop"""
  p, start, goal, line, sdf = PC_.motivating_case()
  S, K = PC_.MOTIV_S, PC_.MOTIV_INTER
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  st, go, sd = t(start), t(goal), t(sdf)
  im = (sd > 0).to(sd.dtype)
  with torch.no_grad():
    one = _planner(PC_.MOTIV_N, 1, PC_.MOTIV_ITERS)
    r = one.forward(t(line), st, go, im, sd)
    assert one.interpolate(r[0], K, sd, eps=0.0).in_collision.tolist() == [True]
    many = _planner(PC_.MOTIV_N, S, PC_.MOTIV_ITERS)
    th, info = many.sample_prior(st, go, S, seed=PC_.MOTIV_SEED, scale=PC_.MOTIV_SCALE, return_noise=True)
    assert th.shape == (1, S, PC_.MOTIV_N, 4) and np.abs(info.noise.cpu().numpy() - PO.all_normals(PC_.MOTIV_SEED, 0, 1, S, PC_.MOTIV_N, 4)).max() <= 1e-13
    rep = lambda a: a.expand(S, *a.shape[1:]).contiguous()
    out = many.forward(th.flatten(0, 1), rep(st), rep(go), rep(im), rep(sd))
    dense = many.interpolate(out[0], K, rep(sd), eps=0.0)
    free = (~dense.in_collision).cpu().numpy()
    err = np.array(out[3], dtype=np.float64).reshape(-1)
  print('collision-free samples: %s, final errors %s' % (np.flatnonzero(free).tolist(), np.round(err[free], 4).tolist()))
  assert free.any() and np.isfinite(err[free]).all()
  assert set(np.flatnonzero(free).tolist()) & set(PC_.MOTIV_FREE)      # among them samples that end free on the CPU oracle's loop as well
  # the selection of INTEGRATION.md: the collision-free sample with the smallest final error
  best = int(np.argmin(np.where(free, err, np.inf)))
  assert free[best] and err[best] < 1.0 and float(IO_.run(p, out[0][best:best + 1].cpu().numpy(), K, sdf, 0.0)[2][0, IO_.COL['in_coll']]) == 0.0
