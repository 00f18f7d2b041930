"""dgp_select_samples on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through the planner.

  * against tests/select_oracle.py: status, order, best, problem_summary and th_best exactly; sample_summary bit for bit the summary of dgp_gp_interpolate run on
    the same B S trajectories;
  * the smallest shapes that reach every path: (n,K) in select_cases.NK (N_d = 3, 49, 129, 257) plus (17,4) (N_d = 81: the 32-lane instantiation, which the four
    do not reach) x (B,S) in select_cases.BS and the hand-made additions, dof 2 and 3, fp32 and fp64 I/O; S = 70 walks passes, S = 17 several wavefronts (asserted
    through dgp_select_launch_shape);
  * shared against per-problem grids, tiled against row-major, env_index against materialised grids, sample-major against problem-major, two runs, two batch
    positions: the same bits; per-problem grids that differ, against the oracle; each output alone; sdf / score / exclude NULL;
  * guard bands and an off-16-byte th / th_best; the timed launch; capture and replay;
  * the planner on the motivating case of tests/prior_cases.py: plan_multistart against the long form, its two grid paths, a bad candidate, a HIP graph."""
import ctypes as C

import numpy as np
import pytest
import torch

import harness
import interp_cases as IC
import interp_oracle as IO_
import prior_cases as PC_
import select_cases as SC
import select_oracle as SO
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTS = ('th_best', 'best', 'order', 'status', 'sample_summary', 'problem_summary')


@pytest.fixture(scope='module')
def be():
  return harness.Backend('hip')


@pytest.fixture(scope='module')
def oracle():
  """the oracle of case (dof, n, K, name), computed once and shared by both I/O types (the inputs are fp32-exact): -> (case, Result)"""
  cache = {}

  def get(dof, n, K, name):
    k = (dof, n, K, name)
    if k not in cache:
      c = dict(SC.all_cases(dof, n))[name] if name == 'additions' else SC.base(dof, n, *[int(v) for v in name.split()[2::2]])
      cache[k] = (c, SO.run(c['p'], c['th'], K, c['sdf'], 0.0, c['score'], c['exclude']))
    return cache[k]
  return get


def sdf_arg(be, solver, sdf, io, tiled):
  sdf = np.asarray(sdf)
  shared, (H, W) = sdf.shape[0] == 1, sdf.shape[-2:]
  if tiled:
    til = harness.tile_np(sdf)
    return solver.sdf_arg(be.to_dev(til, io, name='sdf')[1], H, W, 0 if shared else til[0].size, layout=_capi.DGP_SDF_TILED4)
  return solver.sdf_arg(be.to_dev(sdf, io, name='sdf')[1], H, W, 0 if shared else H * W)


def run(be, c, K, io='f64', sdf='case', tiled=False, sample_major=False, env_index=None, score='case', exclude='case', require_inside=True, want=OUTS, eps=0.0):
  """dgp_select_samples -> {output name: array}, None where not asked for.  sdf: 'case' (the case's shared grid), None, or (G,1,H,W) grids (one per problem, or
  indexed by env_index)"""
  be._keep, be._rec = [], {}
  p = c['p']
  solver = _capi.Solver(harness.config_from_oracle(p, io), api=be.api)
  th = np.asarray(c['th'])
  B, S, n, d = th.shape
  lay = (lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))) if sample_major else (lambda a: a)
  th_p = be.to_dev(lay(th), io, name='th')[1]
  sc = c['score'] if isinstance(score, str) else score
  ex = c['exclude'] if isinstance(exclude, str) else exclude
  sc_p = be.to_dev(lay(sc), io, name='score')[1] if sc is not None else None
  ex_p = be.to_dev(lay(ex), dtype=np.int32, name='exclude')[1] if ex is not None else None
  grid = c['sdf'] if isinstance(sdf, str) else sdf
  arg = None if grid is None else sdf_arg(be, solver, grid, io, tiled)
  ei_p = be.to_dev(env_index, dtype=np.int32, name='env_index')[1] if env_index is not None else None
  shapes = dict(th_best=((B, n, d), io, None), best=((B,), None, np.int32), order=((B, S), None, np.int32), status=((B, S), None, np.int32),
                sample_summary=((B, S, _capi.DGP_DENSE_COUNT), None, np.float64), problem_summary=((B, _capi.DGP_SELECT_COUNT), None, np.float64))
  bufs = {k: (be.empty(shapes[k][0], shapes[k][1], shapes[k][2], name=k) if k in want else (None, None)) for k in OUTS}
  solver.select_samples(B, S, th_p, solver.select_params(K, eps, sample_major, require_inside), sc_p, ex_p, arg, ei_p, stream=be.stream(), **{k: v[1] for k, v in bufs.items()})
  be._done()
  return {k: be.to_np(v[0]) for k, v in bufs.items()}


def interp_summary(be, c, K, io, grids=None, eps=0.0):
  """dgp_gp_interpolate's summary of the B S trajectories of the case, (B,S,6); grids: one per trajectory (B S,1,H,W), default the case's shared grid"""
  be._keep, be._rec = [], {}
  solver = _capi.Solver(harness.config_from_oracle(c['p'], io), api=be.api)
  B, S, n, d = c['th'].shape
  sm, sm_p = be.empty((B * S, _capi.DGP_DENSE_COUNT), dtype=np.float64)
  solver.gp_interpolate(B * S, be.to_dev(c['th'].reshape(B * S, n, d), io)[1], K, sdf_arg(be, solver, c['sdf'] if grids is None else grids, io, False), eps, None, None, sm_p,
                        be.stream())
  return be.to_np(sm).reshape(B, S, -1)


def compare(tag, got, want, c):
  """got: run()'s outputs, want: the oracle's Result -> list of failure strings (every field exact)"""
  bad = []
  for k in ('status', 'order', 'best'):
    if got[k] is not None and not np.array_equal(got[k], getattr(want, k)): bad.append('%s: %s %s, expected %s' % (tag, k, got[k].tolist(), getattr(want, k).tolist()))
  if got['problem_summary'] is not None and not IC.same_bits(got['problem_summary'], want.problem_summary):
    bad.append('%s: problem_summary %s, expected %s' % (tag, got['problem_summary'].tolist(), want.problem_summary.tolist()))
  if got['th_best'] is not None and not IC.same_bits(got['th_best'], want.th_best): bad.append('%s: th_best is not a bit copy of the chosen trajectories' % tag)
  return bad


def same(a, b):
  return all((a[k] is None and b[k] is None) or IC.same_bits(a[k], b[k]) for k in OUTS)


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('dof', [2, 3])
def test_every_shape_against_the_oracle(be, oracle, dof, io):
  bad, lpts = [], set()
  for n, K in SC.NK + (SC.NK32,):
    solver = _capi.Solver(harness.config_from_oracle(SC.base(dof, n, 1, 1)['p'], io), api=be.api)
    lpt = IO_.lpt(IO_.num_dense(n, K))
    lpts.add(lpt)
    assert solver.select_launch_shape(1, K)[0] == lpt == SC.LPT[(n, K)]
    if lpt == 64:
      assert solver.select_launch_shape(70, K)[2] > 1 and solver.select_launch_shape(17, K)[1] > 1      # 70 samples in passes, 17 on several wavefronts
    for name, _ in SC.all_cases(dof, n):
      c, want = oracle(dof, n, K, name)
      got = run(be, c, K, io)
      tag = 'dof %d %s n %d K %d %s' % (dof, io, n, K, name)
      bad += compare(tag, got, want, c)
      if not IC.same_bits(got['sample_summary'], interp_summary(be, c, K, io)): bad.append('%s: sample_summary is not dgp_gp_interpolate\'s summary bit for bit' % tag)
      if not np.array_equal(got['sample_summary'][:, :, IO_.EXACT], want.sample_summary[:, :, IO_.EXACT]): bad.append('%s: sample_summary against the oracle' % tag)
  assert lpts == {16, 32, 64}
  assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_layouts_indexing_runs_and_batch_position_are_bit_equal(be, oracle, io):
  for dof, n, K, name in ((2, 17, 2, 'base B 7 S 4'), (3, 33, 7, 'base B 3 S 17'), (2, 65, 1, 'base B 2 S 70'), (3, 17, 4, 'additions')):
    c, want = oracle(dof, n, K, name)
    B, S = c['th'].shape[:2]
    ref = run(be, c, K, io)
    assert not compare(name, ref, want, c)
    per = np.ascontiguousarray(np.broadcast_to(c['sdf'], (B,) + c['sdf'].shape[1:]))
    more = np.ascontiguousarray(np.broadcast_to(c['sdf'], (B + 2,) + c['sdf'].shape[1:]))
    env = ((np.arange(B) * 3 + 1) % (B + 2)).astype(np.int32)
    for what, kw in (('again', {}), ('tiled shared', dict(tiled=True)), ('per-problem', dict(sdf=per)), ('tiled per-problem', dict(sdf=per, tiled=True)),
                     ('env_index', dict(sdf=more, env_index=env)), ('sample-major', dict(sample_major=True)), ('sample-major per-problem tiled', dict(sample_major=True, sdf=per, tiled=True))):
      assert same(run(be, c, K, io, **kw), ref), (dof, n, K, io, what)
    # the same problems one batch position further on (the last becomes the first): the same bits
    rc = dict(c, th=np.roll(c['th'], 1, 0), score=np.roll(c['score'], 1, 0), exclude=np.roll(c['exclude'], 1, 0))
    rolled = run(be, rc, K, io)
    assert all(IC.same_bits(rolled[k], np.roll(ref[k], 1, 0)) for k in OUTS), (dof, n, K, io, 'rolled')


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_distinct_grids_and_env_index_against_the_oracle(be, io):
  for dof, n, K, (B, S) in ((2, 17, 2, (5, 3)), (3, 33, 7, (3, 17))):
    c = SC.base(dof, n, B, S)
    grids = SC.distinct_grids(c['sdf'], B + 2)
    env = ((np.arange(B) * 3 + 1) % (B + 2)).astype(np.int32)
    for tiled in (False, True):
      got = run(be, c, K, io, sdf=grids[:B], tiled=tiled)
      want = SO.run(c['p'], c['th'], K, grids[:B], 0.0, c['score'], c['exclude'])
      assert not compare('distinct', got, want, c)
      assert IC.same_bits(got['sample_summary'], interp_summary(be, c, K, io, np.repeat(grids[:B], S, axis=0)))
      got = run(be, c, K, io, sdf=grids, env_index=env, tiled=tiled)
      assert same(got, run(be, c, K, io, sdf=grids[env], tiled=tiled))
      assert not compare('env_index', got, SO.run(c['p'], c['th'], K, grids, 0.0, c['score'], c['exclude'], env_index=env), c)
    assert not np.array_equal(SO.run(c['p'], c['th'], K, grids[:B], 0.0, c['score'], c['exclude']).sample_summary, SO.run(c['p'], c['th'], K, c['sdf'], 0.0).sample_summary)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_each_output_alone_and_null_arguments(be, oracle, io):
  for dof, n, K, name in ((2, 17, 2, 'additions'), (3, 65, 1, 'base B 3 S 17')):
    c, want = oracle(dof, n, K, name)
    ref = run(be, c, K, io)
    for k in OUTS:
      only = run(be, c, K, io, want=(k,))
      assert IC.same_bits(only[k], ref[k]) and all(only[j] is None for j in OUTS if j != k), (name, k)
    for what, kw, okw in (('no grid', dict(sdf=None, want=tuple(k for k in OUTS if k != 'sample_summary')), dict(sdf=None)),
                          ('no score', dict(score=None), dict(score=None)), ('no exclude', dict(exclude=None), dict(exclude=None)),
                          ('nothing optional', dict(sdf=None, score=None, exclude=None, want=('th_best', 'best', 'order')), dict(sdf=None, score=None, exclude=None)),
                          ('not inside', dict(require_inside=False), dict(require_inside=False)), ('eps', dict(eps=0.25), dict(eps=0.25))):
      o = dict(sdf=c['sdf'], eps=0.0, score=c['score'], exclude=c['exclude'])
      o.update(okw)
      w = SO.run(c['p'], c['th'], K, o.pop('sdf'), o.pop('eps'), **o)
      assert not compare('%s %s' % (name, what), run(be, c, K, io, **kw), w, c)
  # the hand-made problem without a collision check: nothing collides, the sample that leaves the limits is still tier 1
  c, _ = oracle(2, 17, 2, 'additions')
  got = run(be, c, 2, io, sdf=None, want=('status', 'order'))
  assert not (got['status'] & SO.COLLIDING).any() and got['order'][1].tolist() == [2, 3, 0, 1, 4, 5, 6, 7]


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_guard_bands_and_unaligned_rows(be, oracle, io):
  g = harness.Backend('hip')
  g.guard = True
  calls = 0
  for mis in (False, {'th', 'th_best'}, True):
    g.misalign = mis
    for dof, n, K, name in ((2, 3, 0, 'base B 5 S 3'), (3, 17, 2, 'additions'), (3, 33, 7, 'base B 3 S 17'), (2, 65, 1, 'base B 2 S 70')):
      c, want = oracle(dof, n, K, name)
      ref = run(be, c, K, io)
      assert same(run(g, c, K, io), ref) and same(run(g, c, K, io, sample_major=True), ref), (mis, name)
      lean = run(g, c, K, io, sdf=None, score=None, exclude=None, want=('th_best',))      # every optional pointer NULL
      assert IC.same_bits(lean['th_best'], SO.run(c['p'], c['th'], K).th_best)
      calls += 3
  assert g.guard_checks > 0 and g.input_checks > 0 and g.calls == calls


def test_timed_launch(be, oracle):
  c, want = oracle(2, 17, 2, 'base B 7 S 4')
  timer = _capi.KernelTimer(1, api=be.api)
  timer.arm()
  got = run(be, c, 2, 'f32')
  torch.cuda.synchronize()
  ms = timer.durations_ms()
  assert len(ms) == 1 and 0.0 < ms[0] < 100.0, ms
  assert not compare('timed', got, want, c)


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


def _replayed(call, outs, static_in, other):
  """capture call(static_in) in a HIP graph -> its outputs after a replay on static_in's first content, and after a replay on `other`"""
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
  first = [t.clone() for t in outs(out)]
  static_in.copy_(other)
  graph.replay()
  torch.cuda.synchronize()
  return first, [t.clone() for t in outs(out)]


def test_select_samples_through_the_planner_capture_and_replay(oracle):
  n, K = 17, 2
  c, want = oracle(2, n, K, 'additions')
  c2, want2 = oracle(2, n, K, 'base B 3 S 17')
  c2 = dict(c2, th=c2['th'][:, :8])
  B, S = c['th'].shape[:2]
  planner = _planner(n, B)
  t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
  sd, sc, ex = t(c['sdf']).expand(B, 1, 16, 16), t(c['score']), t(c['exclude'], torch.int32)
  call = lambda th: planner.select_samples(th, sd, score=sc, exclude=ex, num_inter=K, return_order=True)
  outs = lambda r: (r[0], r[1].best, r[1].status, r[1].order, r[1].sample_raw, r[1].raw)
  with torch.no_grad():
    eager, eager2 = call(t(c['th'])), call(t(c2['th']))
    first, second = _replayed(call, outs, t(c['th']).clone(), t(c2['th']))
  assert all(torch.equal(a, b) or (a.dtype.is_floating_point and IC.same_bits(a.cpu().numpy(), b.cpu().numpy())) for a, b in zip(first, outs(eager)))
  assert all(torch.equal(a, b) or (a.dtype.is_floating_point and IC.same_bits(a.cpu().numpy(), b.cpu().numpy())) for a, b in zip(second, outs(eager2)))
  th_best, info = eager
  assert info.best.dtype == torch.int32 and info.solved.dtype == torch.bool and info.solved.tolist() == [True, False, True] and info.num_accepted.tolist() == [5, 0, 4]
  got = dict(th_best=th_best.cpu().numpy(), best=info.best.cpu().numpy(), order=info.order.cpu().numpy(), status=info.status.cpu().numpy(), problem_summary=info.raw.cpu().numpy())
  assert not compare('planner', got, want, c)
  assert info.excluded[0].tolist() == [False] * 7 + [True] and info.non_finite[1].tolist() == [False] * 6 + [True, True] and info.outside[0, 5] and not info.colliding[0].any()
  # float32, sample-major, one grid per problem
  per = t(c['sdf'], torch.float32).expand(B, 1, 16, 16).contiguous()
  tb32, i32 = planner.select_samples(t(c['th'], torch.float32).transpose(0, 1).contiguous(), per, score=sc.float().T.contiguous(), exclude=ex.T.contiguous(), num_inter=K,
                                     sample_major=True)
  assert tb32.dtype == torch.float32 and i32.order is None and np.array_equal(i32.best.cpu().numpy(), want.best) and IC.same_bits(tb32.cpu().numpy(), want.th_best)
  for bad in (lambda: planner.select_samples(t(c['th'])[:, :, :5], sd), lambda: planner.select_samples(t(c['th']), sd, num_inter=1024),
              lambda: planner.select_samples(t(c['th']), sd, score=sc[:, :3]), lambda: planner.select_samples(t(c['th']), None, env_index=ex[:, 0])):
    with pytest.raises(ValueError):
      bad()


def test_plan_multistart_on_the_motivating_case():
  """one disc on the start-goal segment: forward() from the straight line ends in collision; plan_multistart over 16 samples of the prior and the line itself
  reports a solved problem, and its choice is that of the long form -- forward() on all candidates, interpolate(), the selection in torch ops"""
  from dgpmp2_amd.utils.planner_utils import select_samples_torch
  p, start, goal, line, sdf = PC_.motivating_case()
  S, K, n, G = PC_.MOTIV_S, PC_.MOTIV_INTER, PC_.MOTIV_N, PC_.MOTIV_G
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  st, go, sd, ln = t(start), t(goal), t(sdf), t(line)
  im = (sd > 0).to(sd.dtype)
  T = S + 1
  with torch.no_grad():
    one = _planner(n, 1, PC_.MOTIV_ITERS)
    r = one.forward(ln, st, go, im, sd)
    assert one.interpolate(r[0], K, sd, eps=0.0).in_collision.tolist() == [True]
    many = _planner(n, T, PC_.MOTIV_ITERS)
    kw = dict(th_extra=ln[:, None], seed=PC_.MOTIV_SEED, scale=PC_.MOTIV_SCALE, num_inter=K)
    th_best, ms = many.plan_multistart(st, go, sd, S, **kw)
    assert ms.select.solved.tolist() == [True] and th_best.shape == (1, n, 4)
    assert many.interpolate(th_best, K, sd, eps=0.0).in_collision.tolist() == [False]
    assert ms.iters.shape == ms.err_final.shape == ms.spd_info.shape == (1, T) and ms.prior.flags.shape == (1, S) and not ms.spd_info.any()
    # the long form on the same device tensors
    th0 = torch.cat((many.sample_prior(st, go, S, seed=PC_.MOTIV_SEED, scale=PC_.MOTIV_SCALE)[0], ln[:, None]), 1)
    rep = lambda a: a.expand(T, *a.shape[1:]).contiguous()
    out = many.forward(th0.flatten(0, 1), rep(st), rep(go), rep(im), rep(sd))
    dense = many.interpolate(out[0], K, rep(sd), eps=0.0)
    err = torch.tensor(out[3], dtype=torch.float64, device=DEV)
    lb, li = select_samples_torch(out[0].view(1, T, n, 4), sd, err.view(1, T), None, total_time_sec=10.0, sphere_radius=0.4, num_inter=K)
    assert torch.equal(li.colliding.view(-1), dense.in_collision) and torch.equal(li.best, ms.select.best) and torch.equal(lb, th_best)
    free = ~dense.in_collision & (ms.select.status.view(-1) & SO.OUTSIDE == 0)
    assert int(ms.select.best[0]) == int(torch.argmin(torch.where(free, err, torch.full_like(err, float('inf')))))      # INTEGRATION.md's three torch ops
    assert torch.equal(ms.err_final.view(-1), err) and int(ms.select.best[0]) != S                                       # (not the straight line)
    assert torch.equal(ms.select.colliding.view(-1), dense.in_collision) and torch.equal(ms.select.sample_raw.view(T, 6), dense.raw)
    # one grid per problem: three problems on materialised copies of the grid, S + 1 solves of three rows each
    st3, go3, ln3 = st.expand(3, 1, 4).contiguous(), go.expand(3, 1, 4).contiguous(), ln.expand(3, n, 4).contiguous()
    kw3 = dict(kw, th_extra=ln3[:, None])
    tb_s, ms_s = many.plan_multistart(st3, go3, sd.expand(3, 1, G, G), S, **kw3)
    tb_p, ms_p = many.plan_multistart(st3, go3, sd.expand(3, 1, G, G).contiguous(), S, **kw3)
    assert torch.equal(ms_s.select.best, ms_p.select.best) and torch.equal(tb_s, tb_p) and ms_s.select.solved.all() and torch.equal(ms_s.select.order, ms_p.select.order)
    assert torch.equal(ms_s.err_final, ms_p.err_final) and torch.equal(ms_s.iters, ms_p.iters) and ms_p.err_final.shape == (3, T)
    assert len(set(ms_s.select.best.tolist())) > 1 or torch.equal(tb_s[0], tb_s[1])      # problem b draws its own samples (first_problem + b)
    # a candidate forced bad through th_extra is excluded or found non-finite, not raised on
    nan = ln.clone()
    nan[0, n // 2, 0] = float('nan')
    tb_n, ms_n = many.plan_multistart(st, go, sd, S, **dict(kw, th_extra=torch.stack((ln, nan), 1)))
    assert ms_n.select.status.shape == (1, S + 2) and (ms_n.select.non_finite[0, S + 1] or ms_n.select.excluded[0, S + 1])
    assert int(ms_n.select.order[0, -1]) == S + 1 and torch.equal(tb_n, th_best) and ms_n.select.solved.tolist() == [True]
    # float32
    tb32, ms32 = many.plan_multistart(st.float(), go.float(), sd.float(), S, **dict(kw, th_extra=ln[:, None].float()))
    assert tb32.dtype == torch.float32 and ms32.select.solved.tolist() == [True]
    # captured in a HIP graph and replayed: nothing in it synchronises
    call = lambda s: many.plan_multistart(s, go, sd, S, **kw)
    outs = lambda o: (o[0], o[1].select.best, o[1].select.status, o[1].select.order, o[1].select.raw, o[1].err_final, o[1].iters, o[1].spd_info)
    other = st.clone()
    other[0, 0, 1] = 0.75
    eager2 = call(other)
    first, second = _replayed(call, outs, st.clone(), other)
    assert all(torch.equal(a, b) for a, b in zip(first, outs((th_best, ms)))) and all(torch.equal(a, b) for a, b in zip(second, outs(eager2)))
    assert not torch.equal(eager2[0], th_best)
  with pytest.raises(ValueError, match='learn'):
    many.learn_module_fcn = object()
    try: many.plan_multistart(st, go, sd, S)
    finally: many.learn_module_fcn = None


def test_generate_dataset_multistart_keeps_the_environment_the_single_start_drops(tmp_path):
  """tests/select_cases.py's two environments: from the straight line Gauss-Newton stays in the disc of environment 0, so the single start drops it; four samples
  of the prior around the line end free, so multistart=4 keeps it.  Environment 1 is kept either way."""
  from dgpmp2_amd.datasets.problem_generation import generate_dataset
  images = torch.from_numpy(SC.dataset_images()).to(DEV)
  planner = _planner(SC.DATASET_N)
  kw = dict(seed=SC.DATASET_SEED, first_diagonal=True, corner_inset=1.0, max_draws=512, check_inter=SC.DATASET_INTER)
  r0 = generate_dataset(str(tmp_path / 'a'), 'train', images, planner, 1, **kw)
  r4 = generate_dataset(str(tmp_path / 'b'), 'train', images, planner, 1, multistart=SC.DATASET_S, **kw)
  assert not (r0['info'].flags.cpu().numpy() & 8).any() and torch.equal(r0['th_init'], r4['th_init']) and torch.equal(r0['start'], r4['start'])
  assert r0['kept'] == [1] and r0['dropped'] == {0: 'Trajectory is in collision'} and r0['in_coll'].tolist() == [True, False] and 'multistart' not in r0
  assert r4['kept'] == [0, 1] and not r4['dropped'] and r4['in_coll'].tolist() == [False, False] and r4['num_envs'] == 2
  ms = r4['multistart']
  assert ms.select.solved.tolist() == [True, True] and ms.select.status.shape == (2, SC.DATASET_S + 1) and int(ms.select.best[0]) != SC.DATASET_S      # not the straight line
  assert planner.interpolate(r4['th_opt'], SC.DATASET_INTER, r4_grids(images, planner), eps=0.0).in_collision.tolist() == [False, False]
  assert ms.select.colliding[0, SC.DATASET_S] and not ms.select.colliding[0, :SC.DATASET_S].any()


def r4_grids(images, planner):
  from dgpmp2_amd.utils.sdf_utils import sdf_2d_batch
  return sdf_2d_batch(images, padlen=0, res=10.0 / images.shape[-1]).unsqueeze(1)
