"""dgp_gp_interpolate on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through the planner.

  * against tests/interp_oracle.py, which restates the header's operation order: th_dense and dense_cost bit for bit, the count, the first and worst indices and
    in_coll exactly, max penetration bit for bit, avg penetration at parity_cases.TOL_ERR['f64'] (the kernel sums per lane and then over the lanes, the oracle in
    state order); fp32 I/O: the oracle fed the fp32-exact inputs, every stored value rounded once;
  * the smallest shapes that reach every path: n in {2, 3, 17, 65, 130} x K in {0, 1, 2, 4, 7} (all three lanes-per-trajectory instantiations, asserted), B in
    {1, 5, 67} (ragged against 4, 2 and 1 trajectories per wavefront), dof 2 and 3, 16 x 16 and 24 x 16 grids, shared and per-sample, row-major and tiled;
    tests/interp_cases.mixed_batch puts colliding, free, leaving and out-of-grid trajectories side by side in every wavefront;
  * K = 0 against dgp_traj_metrics; shared against per-sample grids, tiled against row-major, two runs, two batch positions: the same bits; each output alone;
  * the motivating case through the planner, generate_dataset(check_inter=7), and capture / replay in a HIP graph."""
import numpy as np
import pytest
import torch

import harness
import interp_cases as IC
import interp_oracle as IO_
import metrics_oracle as MO
import parity_cases as PC
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NS, KS, BS = (2, 3, 17, 65, 130), (0, 1, 2, 4, 7), (1, 5, 67)
GRIDS = ((16, 16), (24, 16))
AVG, MAXP = IO_.COL['avg_penetration'], IO_.COL['max_penetration']


@pytest.fixture(scope='module')
def be():
  return harness.Backend('hip')


def sdf_arg(be, solver, sdf, io, tiled):
  sdf = np.asarray(sdf)
  shared, (H, W) = sdf.shape[0] == 1, sdf.shape[-2:]
  if tiled:
    til = harness.tile_np(sdf)
    return solver.sdf_arg(be.to_dev(til, io)[1], H, W, 0 if shared else til[0].size, layout=_capi.DGP_SDF_TILED4)
  return solver.sdf_arg(be.to_dev(sdf, io)[1], H, W, 0 if shared else H * W)


def run(be, p, th, K, sdf=None, eps=0.0, io='f64', tiled=False, want=(True, True, True)):
  """dgp_gp_interpolate -> (th_dense (B,N_d,d), dense_cost (B,N_d), summary (B,6)) as float64, None where not asked for; sdf (1 | B, 1, H, W) or None"""
  be._keep = []
  solver = _capi.Solver(harness.config_from_oracle(p, io), api=be.api)
  B, n, d = th.shape
  nd = IO_.num_dense(n, K)
  _, th_p = be.to_dev(th, io)
  arg = None if sdf is None else sdf_arg(be, solver, sdf, io, tiled)
  dn, dn_p = be.empty((B, nd, d), io) if want[0] else (None, None)
  co, co_p = be.empty((B, nd), io) if want[1] else (None, None)
  sm, sm_p = be.empty((B, _capi.DGP_DENSE_COUNT), dtype=np.float64) if want[2] else (None, None)
  solver.gp_interpolate(B, th_p, K, arg, eps, dn_p, co_p, sm_p, be.stream())
  return be.to_np(dn), be.to_np(co), be.to_np(sm)


def check(tag, got, want):
  """got / want: (th_dense, dense_cost, summary) -> list of failure strings"""
  bad = []
  for name, g, w in (('th_dense', got[0], want[0]), ('dense_cost', got[1], want[1])):
    if w is not None and not IC.same_bits(g, w):
      k = np.argwhere(~((IC.bits(g) == IC.bits(w)) | (np.isnan(g) & np.isnan(w))))[0]
      bad.append('%s: %s differs from the oracle at %s: %r against %r' % (tag, name, tuple(k), g[tuple(k)], w[tuple(k)]))
  if want[2] is not None:
    g, w = got[2], want[2]
    if not np.array_equal(g[:, IO_.EXACT], w[:, IO_.EXACT]):
      b = np.argwhere((g[:, IO_.EXACT] != w[:, IO_.EXACT]).any(1))[0, 0]
      bad.append('%s: summary of trajectory %d %s, expected %s' % (tag, b, g[b], w[b]))
    if not IC.same_bits(g[:, MAXP], w[:, MAXP]): bad.append('%s: max penetration %s, expected %s' % (tag, g[:, MAXP], w[:, MAXP]))
    e = np.abs(g[:, AVG] - w[:, AVG]) / np.maximum(np.abs(w[:, AVG]), 1e-300)
    e[g[:, AVG] == w[:, AVG]] = 0.0
    if not (e < PC.TOL_ERR['f64']).all(): bad.append('%s: avg penetration rel err %.3g' % (tag, np.nanmax(e)))
  return bad


def per_sample(sdf, B, seed=1):
  """one grid per trajectory: the shared one plus a constant each, fp32-exact"""
  return PC.rnd(sdf + np.random.RandomState(seed).uniform(-0.3, 0.3, (B, 1, 1, 1)), 'f32')


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('dof', [2, 3])
def test_every_shape_against_the_oracle(be, dof, io):
  bad, lpts, seen_coll = [], set(), set()
  full = {(2, 7): 16, (17, 4): 32, (65, 2): 64}      # (n, K) run with every batch size x grid x ownership x layout, one per lanes-per-trajectory count
  for i, n in enumerate(NS):
    for j, K in enumerate(KS):
      nd = IO_.num_dense(n, K)
      lpts.add(IO_.lpt(nd))
      if (n, K) in full:
        assert IO_.lpt(nd) == full[(n, K)]
        combos = [(B, hw, shared, tiled) for B in BS for hw in GRIDS for shared in (True, False) for tiled in (False, True)]
      else:
        c = i * len(KS) + j
        combos = [(BS[c % 3], GRIDS[(c // 3) % 2], (c // 2) % 2 == 0, c % 2 == 1)]
      for B, hw, shared, tiled in combos:
        p, th, sdf = IC.mixed_batch(dof, n, B, hw, seed=n * 8 + K)
        if not shared: sdf = per_sample(sdf, B)
        eps = 0.0 if (n + K) % 2 else 0.25
        summ = nd >= 3
        want = IO_.run(p, th, K, sdf, eps, io)
        got = run(be, p, th, K, sdf, eps, io, tiled, want=(True, True, summ))
        tag = 'dof %d %s n %d K %d B %d grid %s %s %s' % (dof, io, n, K, B, hw, 'shared' if shared else 'per-sample', 'tiled' if tiled else 'row-major')
        bad += check(tag, got, want)
        if summ: seen_coll |= set(want[2][:, IO_.COL['in_coll']].tolist())
        if summ and B >= 5: assert want[2][:, IO_.COL['in_coll']].min() == 0 and want[2][:, IO_.COL['in_coll']].max() == 1, tag      # colliding and free side by side
  assert lpts == {16, 32, 64} and seen_coll == {0.0, 1.0}
  assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_copies_are_bit_copies_and_interpolation_needs_no_grid(be, io):
  """interpolation only (sdf NULL): NaN and -0.0 planted in support states pass through untouched, the rows next to a NaN state are NaN, nothing else moves"""
  for dof, n, K in ((2, 3, 7), (3, 17, 2), (2, 65, 1)):
    B, d = 5, 2 * dof
    p, th, _ = IC.mixed_batch(dof, n, B, (16, 16))
    th[0, 1, 0], th[1, n - 1, d - 1], th[2, 0, 1], th[3, 1, 2] = np.nan, np.nan, -0.0, -0.0
    got = run(be, p, th, K, None, 0.0, io, want=(True, False, False))[0]
    want = IO_.run(p, th, K, None, 0.0, io)[0]
    assert IC.same_bits(got, want), (dof, n, K)
    assert np.array_equal(IC.bits(got[:, ::K + 1])[~np.isnan(th)], IC.bits(th)[~np.isnan(th)]) and np.array_equal(np.isnan(got[:, ::K + 1]), np.isnan(th))
    assert np.signbit(got[2, 0, 1]) and np.signbit(got[3, K + 1, 2])
    assert np.isnan(got[0, 1:2 * (K + 1), 0]).all() and not np.isnan(got[0, :, 1]).any()      # the NaN column of the two intervals around state 1, and no other column


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_k0_is_the_metrics_kernel(be, io):
  for dof, n, B in ((2, 17, 67), (3, 65, 5), (2, 130, 5)):
    p, th, sdf = IC.mixed_batch(dof, n, B, (24, 16), seed=n)
    for tiled in (False, True):
      dn, co, sm = run(be, p, th, 0, sdf, 0.1, io, tiled)
      be._keep = []
      solver = _capi.Solver(harness.config_from_oracle(p, io), api=be.api)
      M, M_p = be.empty((B, _capi.DGP_METRIC_COUNT), dtype=np.float64)
      oe, oe_p = be.empty((B, n), io)
      solver.traj_metrics(B, be.to_dev(th, io)[1], sdf_arg(be, solver, sdf, io, tiled), 0.1, None, M_p, oe_p, be.stream())
      M, oe = be.to_np(M), be.to_np(oe)
      assert IC.same_bits(dn, th) and IC.same_bits(co, oe), (dof, n, io, tiled)
      assert np.array_equal(sm[:, IO_.COL['num_colliding']], M[:, MO.COL['num_penetrating']]) and np.array_equal(sm[:, IO_.COL['in_coll']], M[:, MO.COL['in_coll']])
      assert IC.same_bits(sm[:, MAXP], M[:, MO.COL['max_penetration']])
      assert sm[:, IO_.COL['in_coll']].min() == 0 and sm[:, IO_.COL['in_coll']].max() == 1


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_layouts_ownership_runs_and_batch_position_are_bit_equal(be, io):
  for dof, n, K, B in ((2, 17, 2, 67), (3, 17, 7, 67), (2, 130, 4, 5)):
    p, th, sdf = IC.mixed_batch(dof, n, B, (24, 16), seed=3)
    per = np.ascontiguousarray(np.broadcast_to(sdf, (B,) + sdf.shape[1:]))
    ref = run(be, p, th, K, sdf, 0.0, io)
    assert ref[2][:, 0].min() == 0 and ref[2][:, 0].max() == 1
    for what, kw in (('again', dict(sdf=sdf)), ('tiled shared', dict(sdf=sdf, tiled=True)), ('per-sample', dict(sdf=per)), ('tiled per-sample', dict(sdf=per, tiled=True))):
      got = run(be, p, th, K, kw['sdf'], 0.0, io, kw.get('tiled', False))
      assert all(IC.same_bits(g, r) for g, r in zip(got, ref)), (dof, n, K, io, what)
    # the same trajectories one batch position further on (the last becomes the first): the same bits
    rolled = run(be, p, np.roll(th, 1, 0), K, sdf, 0.0, io)
    assert all(IC.same_bits(g, np.roll(r, 1, 0)) for g, r in zip(rolled, ref)), (dof, n, K, io, 'rolled')
    # each output alone
    for k in range(3):
      only = run(be, p, th, K, sdf, 0.0, io, want=tuple(i == k for i in range(3)))
      assert IC.same_bits(only[k], ref[k]) and all(only[i] is None for i in range(3) if i != k), (dof, n, K, io, k)


def _planner(n, B=1):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)


def test_motivating_case_through_the_planner():
  """the support states clear the disc: trajectory_metrics reports a free trajectory; the path between them crosses it: interpolate(7) reports the collision"""
  p, th, sdf = IC.motivating_case()
  planner = _planner(3)
  for dtype in (torch.float64, torch.float32):
    tht, sdft = torch.from_numpy(th).to(dtype).to(DEV), torch.from_numpy(sdf).to(dtype).to(DEV)
    assert not planner.trajectory_metrics(tht, sdft, eps=0.0).in_collision.any()
    r0 = planner.interpolate(tht, 0, sdft, eps=0.0)
    assert not r0.in_collision.any() and torch.equal(r0.th, tht) and r0.first_colliding.tolist() == [-1]
    r = planner.interpolate(tht, 7, sdft, eps=0.0, return_cost=True)
    want = IO_.run(p, th, 7, sdf, 0.0, 'f64' if dtype is torch.float64 else 'f32')
    assert r.in_collision.tolist() == [True] and 1 <= int(r.first_colliding[0]) <= 7
    assert r.th.shape == (1, 17, 4) and r.th.dtype == dtype and r.cost.dtype == dtype and r.raw.dtype == torch.float64
    assert IC.same_bits(r.th.cpu().numpy(), want[0]) and IC.same_bits(r.cost.cpu().numpy(), want[1]) and np.array_equal(r.raw.cpu().numpy()[:, IO_.EXACT], want[2][:, IO_.EXACT])
    assert int(r.worst_index[0]) == int(want[2][0, IO_.COL['worst_index']]) and float(r.max_penetration[0]) == want[2][0, MAXP] > 0.0
    np.testing.assert_allclose(r.times.cpu().numpy(), IO_.times(p, 7), rtol=0, atol=1e-12)
    # the torch mirror gives the dense trajectory of the kernel to rounding; interpolation alone needs no grid
    from dgpmp2_amd.utils.planner_utils import gp_interpolate_traj
    only = planner.interpolate(tht, 7)
    assert only.raw is None and torch.equal(only.th, r.th)
    assert (gp_interpolate_traj(tht, 10.0, 2, 7) - r.th).abs().max() < (1e-11 if dtype is torch.float64 else 1e-5)


def test_generate_dataset_check_inter_drops_the_straddling_environment(tmp_path):
  """two environments, one diagonal problem each (states at the corners and the centre): in environment 0 a small disc lies on either diagonal between two states, in
  environment 1 the disc lies off both.  The support-state check keeps both; check_inter = 7 drops environment 0."""
  from dgpmp2_amd.datasets.problem_generation import generate_dataset
  S = 32
  c = -5.0 + (10.0 / S) * (np.arange(S) + 0.5)
  X, Y = np.meshgrid(c, c[::-1])
  im = np.ones((2, S, S))
  q = c[9]                                            # -2.03125: a pixel centre, on the diagonals half way between a corner state (+-4) and the centre state
  for cx, cy in ((q, q), (-q, -q), (q, -q), (-q, q)): im[0][(X - cx) ** 2 + (Y - cy) ** 2 <= 0.5 ** 2] = 0.0
  im[1][(X - c[16]) ** 2 + (Y - 3.0) ** 2 <= 0.5 ** 2] = 0.0
  assert (im[0] == 0).sum() == 36 and (im[1] == 0).sum() >= 4
  images = torch.from_numpy(im).to(DEV)
  planner = _planner(3)
  kw = dict(seed=5, first_diagonal=True, corner_inset=1.0, max_draws=512)
  r0 = generate_dataset(str(tmp_path / 'a'), 'train', images, planner, 1, **kw)
  r7 = generate_dataset(str(tmp_path / 'b'), 'train', images, planner, 1, check_inter=7, **kw)
  assert not (r0['info'].flags.cpu().numpy() & 8).any()                      # both problems are the diagonals asked for
  assert torch.equal(r0['th_opt'], r7['th_opt'])
  assert r0['kept'] == [0, 1] and not r0['dropped'] and r0['in_coll'].tolist() == [False, False]
  assert r7['kept'] == [1] and r7['dropped'] == {0: 'Trajectory is in collision'} and r7['in_coll'].tolist() == [True, False] and r7['num_envs'] == 1


def test_interpolate_capture_and_replay():
  n, B, K = 17, 5, 4
  p, th, sdf = IC.mixed_batch(2, n, B, (24, 16), seed=9)
  planner = _planner(n, B)
  tht, sdft = torch.from_numpy(th).to(DEV), torch.from_numpy(sdf).to(DEV).expand(B, 1, 24, 16)
  other = torch.from_numpy(IC.mixed_batch(2, n, B, (24, 16), seed=10)[1]).to(DEV)
  call = lambda t: planner.interpolate(t, K, sdft, eps=0.1, return_cost=True)
  outs = lambda r: (r.th, r.cost, r.raw, r.times)
  with torch.no_grad():
    eager, eager2 = call(tht), call(other)
    static_in = tht.clone()
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
    static_in.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs(out), outs(eager2))) and not torch.equal(eager.th, eager2.th)
  want = IO_.run(p, th, K, sdf, 0.1)
  assert not check('planner', tuple(t.cpu().numpy() for t in outs(eager)[:3]), want)
