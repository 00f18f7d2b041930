"""dgp_heading_lift on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through the planner.

  * supplied turns: every output bit for bit against tests/heading_oracle.py, which restates the header's operation order, and info exactly -- n in {2, 3, 17, 64, 65,
    130, 257, 640} (ragged groups, the three lanes-per-trajectory instantiations and the block loop with its carries), B in {1, 5}, blend in {1, 3, N}, both heading
    modes, both velocity modes, the end modes supplied / tangent / random and two mixed pairs, fp64 and fp32 I/O.  Not the full cross product: every n runs every
    (heading, ends, velocity) combination, each at ONE (B, blend) pair and one window of the case kinds, rotated with the combination and with n; every kind of
    tests/heading_cases.py with a degenerate tangent is run at every n on its own;
  * LINEAR / KEEP against fixture g14_heading_lift (the reference's straight_line_trajb with dof = 3) bit for bit; random ends bit for bit against the oracle's Philox;
  * generated turns: turns_out within TURN_ULPS ulp(pi) of the oracle's, and fed back they reproduce th bit for bit.  The bound is derived, not measured: the cross and
    dot products are bit-identical, so only atan2 differs -- 2 ulp for the device's fp64 library, 1 ulp for the host's, as tests/test_hip_prior.py takes them -- so
    |d turn| <= 3 ulp(pi) (|turn| <= pi); heading i sums i turns and adds base, each sum rounding at the size of the running heading: (i + 2) (3 ulp(pi) +
    ulp(max_j |phi_j|)); ten times that is allowed, as that file allows.  omega gets the sum of its two headings' bounds over (hi - lo) Delta.  fp32 I/O: equal after
    rounding, or adjacent floats -- wherever the fp64 bound is below half a float spacing of the value, which is every heading and every omega that is not itself
    rounding noise; an omega of a straight stretch is a difference of two equal headings, as small as the bound itself, and is held to the bound plus one float
    spacing, which is what rounding two doubles that close can give;
  * purity: a trajectory alone and inside a batch, two batch positions with first_problem shifted, two runs, unaligned buffers, guard bands with every optional
    pointer NULL: the same bits;
  * every DGP_EINVAL case of the header leaves every output untouched; capture / replay in a HIP graph; the timed launch;
  * through the planner, on a g3_c4_xyh-style non-holonomic configuration: init_paths / sample_problems / generate_dataset with a dof 3 planner; the start and
    goal that go to forward() and into the files are rows 0 and N of the lifted initial trajectory, on cases where the goal heading passed in lies a full turn away."""
import ctypes as C

import numpy as np
import pytest
import torch

import harness
import heading_cases as HC
import heading_oracle as HO
import problems_oracle as PR
from dgpmp2_amd import _capi
from oracle import gpmp2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NS = (2, 3, 17, 64, 65, 130, 257, 640)
COMBOS = tuple((h, e, v) for h in ('tangent', 'linear') for e in ('supplied', 'tangent', 'random', ('tangent', 'supplied'), ('random', 'tangent')) for v in ('diff', 'keep')
               if not (h == 'linear' and 'tangent' in ((e,) if isinstance(e, str) else e)))
TURN_ULPS = 3.0
ULP_PI = float(np.spacing(np.pi))


@pytest.fixture(scope='module')
def be():
  return harness.Backend('hip')


def params(n, total_time_sec=HC.T_SEC):
  return O.OracleParams(dof=3, total_time_step=n - 1, total_time_sec=total_time_sec, non_holonomic=True)


def run(be, n, th2, heading='tangent', ends='supplied', velocity='diff', blend=1, hs=None, hg=None, turns=None, seed=0, first_problem=0, io='f64', want_turns=True,
        want_info=True, total_time_sec=HC.T_SEC, p=None, raw_params=None, null=(), batch=None, kept=None):
  """dgp_heading_lift -> (start (B,1,6), goal (B,1,6), th (B,n,6), turns_out (B,n) or None, info (B) or None) as numpy arrays.
  null: names among 'handle', 'params', 'th2', 'start', 'goal', 'th' that go down as NULL (their buffers exist all the same); batch: the batch argument, default
  th2's; kept: a list that receives the outputs as they are read back, also when the call raises."""
  be._keep, be._rec = [], {}
  solver = _capi.Solver(harness.config_from_oracle(p if p is not None else params(n, total_time_sec), io), api=be.api)
  B = th2.shape[0]
  se, ge = (ends, ends) if isinstance(ends, str) else ends
  hp = raw_params if raw_params is not None else _capi.Solver.heading_params(HO.HEADING[heading], HO.END[se], HO.END[ge], HO.VEL[velocity], blend, seed, first_problem)
  _, t2_p = be.to_dev(th2, io, name='th2')
  _, hs_p = be.to_dev(hs, dtype=np.float64, name='start_heading')
  _, hg_p = be.to_dev(hg, dtype=np.float64, name='goal_heading')
  _, ti_p = be.to_dev(turns, dtype=np.float64, name='turns_in')
  st, st_p = be.empty((B, 1, 6), io, name='start')
  go, go_p = be.empty((B, 1, 6), io, name='goal')
  th, th_p = be.empty((B, n, 6), io, name='th')
  to, to_p = be.empty((B, n), dtype=np.float64, name='turns_out') if want_turns else (None, None)
  info, info_p = be.empty((B,), dtype=np.int32, name='info') if want_info else (None, None)
  try:
    if null or batch is not None:
      a = dict(handle=solver.handle, params=C.byref(hp), th2=t2_p, start=st_p, goal=go_p, th=th_p)
      assert set(null) <= set(a)
      for name in null: a[name] = None
      be.api.check(be.api.heading_lift(a['handle'], B if batch is None else batch, a['params'], a['th2'], hs_p, hg_p, ti_p, a['start'], a['goal'], a['th'], to_p, info_p,
                                       be.stream()))
    else: solver.heading_lift(B, hp, t2_p, st_p, go_p, th_p, hs_p, hg_p, ti_p, to_p, info_p, be.stream())
  finally:
    res = be.to_np(st), be.to_np(go), be.to_np(th), be.to_np(to), be.to_np(info)
    if kept is not None: kept.extend(res)
    be._done()
  return res


def same(got, want):
  return all(HC.same_bits(a, b) for a, b in zip(got[:4], want[:4])) and np.array_equal(got[4], want[4])


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_supplied_turns_bit_for_bit(be, io):
  bad, seen = [], set()
  for i, n in enumerate(NS):
    N = n - 1
    pairs = tuple((B, blend) for B in (1, 5) for blend in sorted({1, min(3, N), N}))
    for c, (heading, ends, velocity) in enumerate(COMBOS):
      B, blend = pairs[(c + i) % len(pairs)]
      th2, names = HC.batch(n, B, c + i, io)
      hs, hg = HC.headings(B, 100 * n + c)
      turns = HO.run(th2, HC.T_SEC, heading, ends, velocity, blend, hs, hg, None, 11, 1 << 33, io)[3]      # the oracle's own atan2; any values would do
      want = HO.run(th2, HC.T_SEC, heading, ends, velocity, blend, hs, hg, turns, 11, 1 << 33, io)
      got = run(be, n, th2, heading, ends, velocity, blend, hs, hg, turns, 11, 1 << 33, io)
      tag = '%s n %d B %d blend %d %s %s %s %s' % (io, n, B, blend, heading, ends, velocity, names)
      for name, a, b in zip(('start', 'goal', 'th', 'turns_out'), got[:4], want[:4]):
        if not HC.same_bits(a, b):
          k = tuple(np.argwhere((HC.bits(a) != HC.bits(b)) & ~(np.isnan(a) & np.isnan(b)))[0])
          bad.append('%s: %s differs from the oracle at %s: %r against %r' % (tag, name, k, a[k], b[k]))
      if not np.array_equal(got[4], want[4]): bad.append('%s: info %s, expected %s' % (tag, got[4], want[4]))
      seen |= set(want[4].tolist())
    # every kind with a degenerate tangent, at every n
    th2 = np.stack([HC.case(k, n, io) for k in HC.DEGENERATE])
    hs, hg = HC.headings(len(HC.DEGENERATE), n)
    blend = max(1, N // 4)
    turns = HO.run(th2, HC.T_SEC, 'tangent', 'supplied', 'diff', blend, hs, hg, None, io=io)[3]
    want = HO.run(th2, HC.T_SEC, 'tangent', 'supplied', 'diff', blend, hs, hg, turns, io=io)
    got = run(be, n, th2, 'tangent', 'supplied', 'diff', blend, hs, hg, turns, io=io)
    if not same(got, want): bad.append('%s n %d degenerate kinds: info %s expected %s, th equal %s' % (io, n, got[4], want[4], HC.same_bits(got[2], want[2])))
    seen |= set(want[4].tolist())
  assert not bad, '\n'.join(bad[:20])
  bits = 0
  for v in seen: bits |= v
  assert bits == 15 and 0 in seen      # every info bit was met, and clean trajectories


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_linear_keep_is_the_reference_straight_line(be, golden, io):
  g = golden('g14_heading_lift')
  for k, c in enumerate(g['cases']):
    n, T = int(c.split()[0]), float(g['c%d_T' % k])
    s, go, ref = g['c%d_start' % k], g['c%d_goal' % k], g['c%d_th' % k]
    th2 = np.stack([PR.straight_line(s[b, 0, :2], go[b, 0, :2], n, T) for b in range(s.shape[0])])
    hs, hg = s[:, 0, 2].copy(), go[:, 0, 2].copy()
    got = run(be, n, HO.rnd(th2, io), 'linear', 'supplied', 'keep', 1, hs, hg, io=io, total_time_sec=T)
    if io == 'f64': assert HC.same_bits(got[2], ref), c      # the reference's own output
    assert same(got, HO.run(HO.rnd(th2, io), T, 'linear', 'supplied', 'keep', 1, hs, hg, io=io)), c
    assert not got[3].any() and not got[4].any()


def test_random_ends_bit_for_bit(be):
  for n, B, seed, first in ((17, 5, 0, 0), (64, 3, (1 << 63) + 12345, (1 << 32) - 1), (130, 2, 7, 1 << 40)):
    th2, _ = HC.batch(n, B, 0)
    for heading, velocity in (('linear', 'keep'), ('linear', 'diff')):      # no transcendental anywhere: every output
      got = run(be, n, th2, heading, 'random', velocity, 1, seed=seed, first_problem=first)
      assert same(got, HO.run(th2, HC.T_SEC, heading, 'random', velocity, 1, seed=seed, first_problem=first)), (n, heading, velocity)
    got = run(be, n, th2, 'tangent', 'random', 'diff', 3, seed=seed, first_problem=first)      # theta_0 is theta_s itself
    assert HC.same_bits(got[0][:, 0, 2], np.array([HO.random_ends(seed, first + b)[0] for b in range(B)]))


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_generated_turns(be, io):
  for n, B, ends, velocity in ((17, 5, 'supplied', 'diff'), (64, 5, 'tangent', 'diff'), (65, 5, ('random', 'supplied'), 'diff'), (640, 2, 'supplied', 'keep'), (3, 5, 'supplied', 'diff')):
    N, blend = n - 1, max(1, (n - 1) // 4)
    th2, names = HC.batch(n, B, 0, io)      # arc, s_curve, staircase, corner, reversal
    hs, hg = HC.headings(B, n)
    got = run(be, n, th2, 'tangent', ends, velocity, blend, hs, hg, None, 3, 9, io)
    want = HO.run(th2, HC.T_SEC, 'tangent', ends, velocity, blend, hs, hg, None, 3, 9, io)
    assert np.array_equal(got[4], want[4]), (n, got[4], want[4])
    assert np.abs(got[3] - want[3]).max() <= TURN_ULPS * ULP_PI, (n, np.abs(got[3] - want[3]).max() / ULP_PI)
    # fed back, the turns reproduce every output bit for bit, and turns_out is then a copy; the oracle fed the same turns agrees as well
    again = run(be, n, th2, 'tangent', ends, velocity, blend, hs, hg, got[3], 3, 9, io)
    assert same(again, got), n
    assert same(got, HO.run(th2, HC.T_SEC, 'tangent', ends, velocity, blend, hs, hg, got[3], 3, 9, io)), n
    # the headings and omega against the oracle's own turns, inside the derived bound
    exact = HO.run(th2, HC.T_SEC, 'tangent', ends, velocity, blend, hs, hg, None, 3, 9, 'f64')      # unrounded fp64 headings
    phi_max = np.abs(exact[2][:, :, 2]).max(1) + np.pi      # the blend terms are at most pi away from phi
    i = np.arange(n)
    bound = 10.0 * (i[None] + 2) * (TURN_ULPS * ULP_PI + np.spacing(phi_max)[:, None])      # (B,n)
    lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, N)
    den = (hi - lo) * (HC.T_SEC / N)
    wb = (bound[:, hi] + bound[:, lo]) / den[None] if velocity == 'diff' else (bound[:, [N]] + bound[:, [0]]) / HC.T_SEC + 0 * den[None]
    assert HC.same_bits(got[2][:, :, [0, 1, 3, 4]], want[2][:, :, [0, 1, 3, 4]])
    for col, tol in ((2, bound), (5, wb)):
      a, b = got[2][:, :, col], want[2][:, :, col]
      if io == 'f64':
        print('%s n %d column %d: max |difference| / bound %.3g' % (io, n, col, (np.abs(a - b) / tol).max()))
        assert (np.abs(a - b) <= tol).all(), (n, col, (np.abs(a - b) / tol).max())
      else:
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        adjacent = (a32 == b32) | (np.nextafter(a32, b32) == b32)
        # two doubles within tol of each other round to floats within tol + one float spacing; where tol is below half a float spacing of the value that IS "equal
        # after rounding, or adjacent floats", and it is asserted in that form there (an omega of a straight stretch is itself of the size of tol: no float is adjacent)
        assert (np.abs(a - b) <= tol + np.spacing(np.maximum(np.abs(a32), np.abs(b32))).astype(np.float64)).all(), (n, col)
        resolved = tol < 0.5 * np.spacing(np.abs(b32)).astype(np.float64)
        assert adjacent[resolved].all() and resolved.any(), (n, col)
    assert np.isfinite(got[2]).all()


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_purity(be, io):
  for n, B, ends in ((17, 5, 'random'), (64, 5, 'supplied'), (130, 5, ('random', 'tangent')), (2, 5, 'random')):
    blend = max(1, (n - 1) // 4)
    th2, _ = HC.batch(n, B, 3, io)
    hs, hg = HC.headings(B, n)
    sub = lambda a, sl: None if a is None else a[sl]
    ref = run(be, n, th2, 'tangent', ends, 'diff', blend, hs, hg, None, 5, 10, io)
    assert same(run(be, n, th2, 'tangent', ends, 'diff', blend, hs, hg, None, 5, 10, io), ref), (n, 'two runs')
    alone = run(be, n, th2[2:3], 'tangent', ends, 'diff', blend, hs[2:3], hg[2:3], None, 5, 12, io)
    assert same(alone, [a[2:3] for a in ref]), (n, 'alone')
    moved = run(be, n, th2[1:], 'tangent', ends, 'diff', blend, hs[1:], hg[1:], None, 5, 11, io)
    assert same(moved, [a[1:] for a in ref]), (n, 'batch position')
    be.misalign = True      # every buffer one element past a 16-byte boundary: the element-wise loads and stores
    try: mis = run(be, n, th2, 'tangent', ends, 'diff', blend, hs, hg, None, 5, 10, io)
    finally: be.misalign = False
    assert same(mis, ref), (n, 'unaligned')


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_guard_bands_with_the_optional_pointers_null(io):
  g = harness.Backend('hip')
  g.guard = True
  for mis in (False, True):
    g.misalign = mis
    for n, B in ((3, 5), (17, 3), (64, 5), (65, 2), (257, 1)):
      blend = max(1, (n - 1) // 4)
      th2, _ = HC.batch(n, B, n, io)
      hs, hg = HC.headings(B, n)
      bare = run(g, n, th2, 'tangent', ('tangent', 'random'), 'diff', blend, io=io, want_turns=False, want_info=False)      # every optional pointer NULL
      full = run(g, n, th2, 'tangent', ('tangent', 'random'), 'diff', blend, io=io)
      assert all(HC.same_bits(a, b) for a, b in zip(bare[:3], full[:3]))
      turns = full[3]
      assert same(run(g, n, th2, 'tangent', 'supplied', 'keep', blend, hs, hg, turns, io=io), HO.run(th2, HC.T_SEC, 'tangent', 'supplied', 'keep', blend, hs, hg, turns, io=io))
  assert g.guard_checks > 0 and g.input_checks > 0 and g.calls == 30


def test_every_einval_case_launches_nothing():
  """Every DGP_EINVAL case of the header, each with real device buffers for every argument it does not make NULL, between guard bands: the error code, and every
  output still NaN / -1 as it was filled (a launch writes every output, always) with its guard bands untouched."""
  g = harness.Backend('hip')
  g.guard = True
  n, B = 17, 2
  th2, _ = HC.batch(n, B, 0)
  hs, hg = HC.headings(B, 1)
  P = _capi.Solver.heading_params
  L, Tn, SUP, ETAN, RND = _capi.DGP_HEADING_LINEAR, _capi.DGP_HEADING_TANGENT, _capi.DGP_END_SUPPLIED, _capi.DGP_END_TANGENT, _capi.DGP_END_RANDOM
  planar = O.OracleParams(dof=2, total_time_step=n - 1)
  ok = P(blend=4)
  cases = [dict(raw_params=ok, null=('handle',)), dict(raw_params=ok, null=('params',)), dict(raw_params=ok, null=('th2',)), dict(raw_params=ok, null=('start',)),
           dict(raw_params=ok, null=('goal',)), dict(raw_params=ok, null=('th',)),
           dict(raw_params=ok, p=planar),                                                       # dof != 3
           dict(raw_params=ok, batch=0), dict(raw_params=ok, batch=-1),                         # batch < 1
           dict(raw_params=P(heading_mode=2, blend=4)), dict(raw_params=P(heading_mode=-1, blend=4)), dict(raw_params=P(velocity_mode=2, blend=4)),
           dict(raw_params=P(velocity_mode=-1, blend=4)), dict(raw_params=P(start_end=3, blend=4)), dict(raw_params=P(goal_end=7, blend=4)),
           dict(raw_params=P(start_end=-1, blend=4)),                                           # unknown modes
           dict(raw_params=P(blend=0)), dict(raw_params=P(blend=n)), dict(raw_params=P(blend=-3)),      # blend outside 1 .. N
           dict(raw_params=P(L, ETAN, SUP, blend=4)), dict(raw_params=P(L, SUP, ETAN, blend=4)),        # tangent ends under the linear rule
           dict(raw_params=P(Tn, SUP, RND, blend=4), hs=None), dict(raw_params=P(Tn, RND, SUP, blend=4), hg=None),      # a supplied end without its array
           dict(raw_params=P(L, SUP, SUP, blend=4), hs=None, hg=None)]
  for io in ('f64', 'f32'):
    for kw in cases:
      args = dict(hs=hs, hg=hg)
      args.update(kw)
      outs = []
      with pytest.raises(_capi.DgpError) as e:
        run(g, n, th2, io=io, kept=outs, **args)
      assert e.value.code == _capi.DGP_EINVAL, (io, kw)
      assert len(outs) == 5 and all(o is not None for o in outs), (io, kw)
      assert all(np.isnan(o).all() for o in outs[:4]) and (outs[4] == -1).all(), (io, kw, [int(np.isfinite(o).sum()) for o in outs[:4]], outs[4])
  assert g.calls == 2 * len(cases) and g.guard_checks >= 5 * g.calls
  # the same buffers and the valid parameters do launch: the fill is what a launch overwrites
  good = run(g, n, th2, raw_params=ok, hs=hs, hg=hg)
  assert all(np.isfinite(o).all() for o in good[:4]) and (good[4] >= 0).all()


def _planner(n, B=1, G=64, max_iters=5):
  """the g3_c4_xyh configuration: the non-holonomic x-y-heading robot"""
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobotXYH
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(3, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01), 'K_d': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 3, 'state_dim': 6, 'total_time_sec': 10.0, 'total_time_step': n - 1, 'non_holonomic': True}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': max_iters, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobotXYH(t(0.4), use_cuda=True, batch_size=B, num_traj_states=n), batch_size=B, use_cuda=True)


def _planar_planner(n, B=1):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 5, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)


def test_lift_capture_replay_and_timed_launch(be):
  n, B = 64, 5
  planner = _planner(n, B)
  a, _ = HC.batch(n, B, 0)
  b, _ = HC.batch(n, B, 2)
  hs, hg = HC.headings(B, 4)
  ta, tb, ths, thg = (torch.from_numpy(v).to(DEV) for v in (a, b, hs, hg))
  call = lambda t: planner.lift_headings(t, start_heading=ths, goal_heading=thg, blend=7, return_turns=True)
  outs = lambda r: (r[0], r[1], r[2], r[3].flags, r[3].turns)
  with torch.no_grad():
    eager, eager2 = call(ta), call(tb)
    static_in = ta.clone()
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
    assert all(torch.equal(x, y) for x, y in zip(outs(out), outs(eager)))
    static_in.copy_(tb)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs(out), outs(eager2))) and not torch.equal(eager[2], eager2[2])
  turns = eager[3].turns.cpu().numpy()
  want = HO.run(a, 10.0, 'tangent', 'supplied', 'diff', 7, hs, hg, turns)
  assert all(HC.same_bits(x.cpu().numpy(), y) for x, y in zip(eager[:3], want[:3])) and np.array_equal(eager[3].flags.cpu().numpy(), want[4])
  # the torch mirror with the kernel's turns: on the host the same bits; on the device torch's own kernels are free to contract a multiply-add, so only close
  from dgpmp2_amd.utils.planner_utils import heading_lift_torch
  mirror = heading_lift_torch(ta.cpu(), 10.0, ths.cpu(), thg.cpu(), blend=7, turns=eager[3].turns.cpu())
  assert all(torch.equal(x, y.cpu()) for x, y in zip(mirror[:3], eager[:3])) and torch.equal(mirror[4], eager[3].flags.cpu())
  on_dev = heading_lift_torch(ta, 10.0, ths, thg, blend=7, turns=eager[3].turns)
  worst = max(float((x - y).abs().max()) for x, y in zip(on_dev[:3], eager[:3]))
  print('torch mirror on the device against the kernel: max |difference| %.3e' % worst)
  assert worst <= 1e-12 and torch.equal(on_dev[4], eager[3].flags)
  # host tensors raise; so does a planar planner
  with pytest.raises(RuntimeError): planner.lift_headings(ta.cpu(), start_heading=ths, goal_heading=thg)
  with pytest.raises(ValueError): _planar_planner(n, B).plan_layer.heading_lift(ta, _capi.Solver.heading_params(blend=7))
  # the timed launch
  timer = _capi.KernelTimer(1, api=be.api)
  timer.arm()
  run(be, n, a, 'tangent', 'supplied', 'diff', 7, hs, hg, io='f32')
  torch.cuda.synchronize()
  ms = timer.durations_ms()
  assert len(ms) == 1 and 0.0 < ms[0] < 100.0, ms


# ---- through the planner: one disc between start and goal on a 64 x 64 grid ------------------------------------------------------------------------------------------
DISC_N, DISC_G = 33, 64


def _disc_scene(B=2):
  sdf = O.circles_sdf(DISC_G, ((0.0, 0.0, 1.2),))[None, None]
  start = np.array([[[-3.5, -0.3, 0.4, 0.0, 0.0, 0.0]], [[-3.0, 2.5, -2.0, 0.0, 0.0, 0.0]]])[:B]
  goal = np.array([[[3.5, 0.2, 5.0, 0.0, 0.0, 0.0]], [[3.2, -2.4, 5.0, 0.0, 0.0, 0.0]]])[:B]
  return sdf, start, goal


def nonholonomic_error(th):
  return th[..., 4] * np.cos(th[..., 2]) - th[..., 3] * np.sin(th[..., 2])


def test_init_paths_with_a_dof3_planner():
  """The tangent lift of the shortcut grid path around one disc: planar columns bit for bit those of the dof 2 call, a vanishing non-holonomic error outside the
  blend zones, a lower total error than the reference's linear / keep lift of the same path, and a forward() that accepts the problem.  The case was fixed on the CPU
  first: tests/paths_oracle.py and tests/shortcut_oracle.py give the path, tests/heading_oracle.py the two lifts, oracle/gpmp2_oracle.py (plan_layer_forward's
  error, K_d = 0.01) the errors -- tangent / diff 133.2 and 116.4 against linear / keep 193.5 and 240.4 for the two problems; the non-holonomic mean square outside
  the blend zones is 4e-33 there, against 0.19 for the linear rule."""
  from dgpmp2_amd.datasets import problem_generation as PG
  n, B = DISC_N, 2
  sdf, start, goal = _disc_scene(B)
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  sd, st, go = t(sdf), t(start), t(goal)
  xyh, planar = _planner(n, B), _planar_planner(n, B)
  planar4 = lambda c: torch.cat((c[..., :2], torch.zeros_like(c[..., :2])), -1)
  with torch.no_grad():
    th2, info2 = PG.init_paths(planar, sd, planar4(st), planar4(go), shortcut=True)
    th, info = PG.init_paths(xyh, sd, st, go, shortcut=True)
    assert tuple(th.shape) == (B, n, 6) and info.heading is not None and info.shortcut is not None and torch.equal(info.flags, info2.flags)
    assert torch.equal(th[..., :2], th2[..., :2])
    assert not bool(info.fell_back.any()) and int(info.heading.flags.max()) & ~HO.SHARP_TURN == 0
    blend = max(1, (n - 1) // 4)
    h = th.cpu().numpy()
    inner = h[:, blend + 1:n - 1 - blend]
    vmax2 = (h[..., 3] ** 2 + h[..., 4] ** 2).max()
    mse = (nonholonomic_error(inner) ** 2).mean()
    print('non-holonomic mse outside the blend zones %.3e, max |v|^2 %.3e' % (mse, vmax2))
    assert mse < 1e-20 * vmax2
    assert h[:, 0, 2].tolist() == start[:, 0, 2].tolist() and np.abs(np.sin((h[:, -1, 2] - goal[:, 0, 2]) / 2)).max() < 1e-15
    # against the reference's rule on the same path
    s_l, g_l, th_lin, _ = xyh.lift_headings(th2, start_heading=st[:, 0, 2], goal_heading=go[:, 0, 2], heading='linear', velocity='keep')
    s_t, g_t, th_tan, _ = xyh.lift_headings(th2, start_heading=st[:, 0, 2], goal_heading=go[:, 0, 2])
    assert torch.equal(th_tan, th)
    rep = sd.expand(B, -1, -1, -1).contiguous()
    im = (rep > 0).to(rep.dtype)
    err = lambda a: np.array(a.cpu().numpy(), dtype=np.float64).reshape(-1)
    xyh.forward(th_lin, s_l, g_l, im, rep)
    e_lin = err(xyh.error_batch(th_lin, rep))      # (the start and goal of the forward() just made)
    out = xyh.forward(th_tan, s_t, g_t, im, rep)
    e_tan = err(xyh.error_batch(th_tan, rep))
    print('error_batch: tangent lift %s, linear / keep lift %s' % (e_tan, e_lin))
    assert (e_tan < e_lin).all()
    assert torch.isfinite(out[0]).all() and tuple(out[0].shape) == (B, n, 6) and np.isfinite(np.array(out[3], dtype=np.float64)).all()
    # the new keywords reach the lift, and a planar planner refuses them
    th_k, info_k = PG.init_paths(xyh, sd, st, go, shortcut=True, heading='linear', velocity='keep')
    assert torch.equal(th_k, th_lin)
    with pytest.raises(TypeError): PG.init_paths(planar, sd, planar4(st), planar4(go), heading='linear')
    # shortcut_paths on its own
    th_g, info_g = PG.init_paths(xyh, sd, st, go, path_cap=4 * (DISC_G + DISC_G))
    th_s, info_s = PG.shortcut_paths(xyh, sd, st, go, th_g, info_g)
    assert torch.equal(th_s, th) and info_s.heading is not None


def test_sample_problems_and_generate_dataset_with_a_dof3_planner(tmp_path):
  from dgpmp2_amd.datasets import problem_generation as PG
  from dgpmp2_amd.datasets.planning_dataset import PlanningDataset
  n = 17
  xyh, planar = _planner(n, 4, max_iters=3), _planar_planner(n, 4)
  sdf = torch.from_numpy(O.circles_sdf(32, ((0.5, -0.5, 1.0),))[None, None]).to(DEV)
  with torch.no_grad():
    a = PG.sample_problems(xyh, sdf, 4, seed=3, first_problem=20, init='grid_path', ends='random')
    b = PG.sample_problems(xyh, sdf, 2, seed=3, first_problem=22, init='grid_path', ends='random')
    assert tuple(a[0].shape) == (4, 1, 6) and tuple(a[2].shape) == (4, n, 6) and a[3].heading is not None
    assert all(torch.equal(x[2:], y) for x, y in zip(a[:3], b[:3]))      # a pure function of (seed, first_problem + b)
    p2 = PG.sample_problems(planar, sdf, 4, seed=3, first_problem=20, init='grid_path')
    assert torch.equal(a[2][..., :2], p2[2][..., :2]) and torch.equal(a[0][..., :2], p2[0][..., :2]) and p2[3].heading is None
    hs = a[0][:, 0, 2].cpu().numpy()
    assert HC.same_bits(hs, np.array([HO.random_ends(3, 20 + k)[0] for k in range(4)]))
    with pytest.raises(TypeError): PG.sample_problems(planar, sdf, 4, ends='random')
    # the generation chain: 2 environments of 32 x 32, 2 problems each
    images = torch.ones(2, 32, 32, dtype=torch.float64, device=DEV)
    images[0, 12:18, 12:18] = 0.0
    images[1, 6:10, 20:26] = 0.0
    gen = _planner(n, 4, max_iters=3)
    r = PG.generate_dataset(str(tmp_path), 'train', images, gen, 2, seed=1, init='shortcut_path', require_collision_free=False)
  assert r['num_envs'] == 2 and tuple(r['th_opt'].shape) == (4, n, 6) and tuple(r['start'].shape) == (4, 1, 6) and r['path_info'].heading is not None
  ds = PlanningDataset(str(tmp_path), 'train')
  assert len(ds) == 4
  for k in range(4):
    s = ds[k]
    assert tuple(s['th_opt'].shape) == (n, 6) and tuple(s['start'].shape) == (1, 6) and tuple(s['goal'].shape) == (1, 6)
    assert np.array_equal(s['th_opt'].numpy(), r['th_opt'][k].cpu().numpy()) and np.array_equal(s['start'].numpy(), r['start'][k].cpu().numpy())


def test_a_dof3_init_paths_carries_the_start_and_goal_of_its_own_path():
  """The goal heading a caller passes in and the one the lifted path arrives with can lie a full turn apart: start heading 2.5, goal heading -2.7 on the disc scene.
  Fixed on the CPU first (tests/paths_oracle.py, tests/shortcut_oracle.py, tests/heading_oracle.py): the shortcut path of problem 0 arrives with 3.5832 = -2.7 + 2 pi,
  where the straight line between the same points keeps -2.7; problem 1 the other way round (-2.7 against 3.5832).  info.heading.start / .goal are rows 0 and N of the
  returned trajectory bit for bit, and they are what forward() takes."""
  from dgpmp2_amd.datasets import problem_generation as PG
  n, B = DISC_N, 2
  sdf, start, goal = _disc_scene(B)
  start[:, 0, 2], goal[:, 0, 2] = 2.5, -2.7
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  sd, st, go = t(sdf), t(start), t(goal)
  xyh = _planner(n, B)
  line = t(np.stack([PR.straight_line(start[b, 0, :2], goal[b, 0, :2], n, 10.0) for b in range(B)]))
  with torch.no_grad():
    g_line = xyh.lift_headings(line, start_heading=st[:, 0, 2], goal_heading=go[:, 0, 2])[1]
    th, info = PG.init_paths(xyh, sd, st, go, shortcut=True)
    hs, hg = info.heading.start, info.heading.goal
    assert tuple(hs.shape) == (B, 1, 6) and tuple(hg.shape) == (B, 1, 6) and hs.dtype == th.dtype
    assert torch.equal(hg[:, 0, :3], th[:, -1, :3]) and torch.equal(hs[:, 0, :3], th[:, 0, :3]) and not bool(hg[..., 3:].any()) and not bool(hs[..., 3:].any())
    assert torch.equal(hs[:, 0, 2], st[:, 0, 2])
    arrive, straight = hg[:, 0, 2].cpu().numpy(), g_line[:, 0, 2].cpu().numpy()
    print('goal heading: passed in %s, of the path %s, of the straight line %s' % (goal[:, 0, 2], arrive, straight))
    assert np.abs(arrive - np.array([-2.7 + HO.TWO_PI, -2.7])).max() < 1e-12 and np.abs(straight - np.array([-2.7, -2.7 + HO.TWO_PI])).max() < 1e-12
    assert arrive[0] != goal[0, 0, 2] and arrive[1] == goal[1, 0, 2]
    # the grid path and shortcut_paths on its own carry theirs as well
    th_g, info_g = PG.init_paths(xyh, sd, st, go, path_cap=4 * (DISC_G + DISC_G))
    assert torch.equal(info_g.heading.goal[:, 0, :3], th_g[:, -1, :3]) and torch.equal(info_g.heading.start[:, 0, :3], th_g[:, 0, :3])
    th_s, info_s = PG.shortcut_paths(xyh, sd, info_g.heading.start, info_g.heading.goal, th_g, info_g)
    assert torch.equal(th_s, th) and torch.equal(info_s.heading.goal, hg) and torch.equal(info_s.heading.start, hs)
    rep = sd.expand(B, -1, -1, -1).contiguous()
    out = xyh.forward(th, hs, hg, (rep > 0).to(rep.dtype), rep)
    assert torch.isfinite(out[0]).all()


WINDING_SEED = 3      # 5 of its 16 problems (1-5 of 16 for each of the seeds 1 .. 6)


def test_generate_dataset_gives_forward_the_goal_its_initial_path_arrives_with(tmp_path):
  """generate_dataset samples the problems on straight lines and then lifts the grid / shortcut paths: 'start' and 'goal' -- what forward() got and what the files
  hold -- are rows 0 and N of 'th_init' bit for bit, on a seed where for some problem the straight line's goal heading (what sample_problems returned) lies a full
  turn from the path's."""
  from dgpmp2_amd.datasets import problem_generation as PG
  from dgpmp2_amd.datasets.planning_dataset import PlanningDataset
  from dgpmp2_amd.utils.sdf_utils import sdf_2d_batch
  n, E, P = 17, 2, 8
  images = torch.ones(E, 32, 32, dtype=torch.float64, device=DEV)
  images[0, 11:21, 11:21] = 0.0
  images[1, 8:24, 13:19] = 0.0
  gen = _planner(n, E * P, max_iters=2)
  with torch.no_grad():
    r = PG.generate_dataset(str(tmp_path), 'train', images, gen, P, seed=WINDING_SEED, first_diagonal=False, init='shortcut_path', require_collision_free=False)
    assert r['num_envs'] == E and r['kept'] == [0, 1]
    start, goal, th_init = r['start'], r['goal'], r['th_init']
    assert tuple(goal.shape) == (E * P, 1, 6) and tuple(th_init.shape) == (E * P, n, 6)
    assert torch.equal(goal[:, 0, :3], th_init[:, -1, :3]) and torch.equal(start[:, 0, :3], th_init[:, 0, :3])
    assert torch.equal(goal[:, 0, 2], th_init[:, -1, 2])      # (the review's line)
    assert torch.equal(goal, r['path_info'].heading.goal) and torch.equal(start, r['path_info'].heading.start)
    # the straight lines of the same problems
    sdf = sdf_2d_batch(images, padlen=0, res=10.0 / 32).unsqueeze(1)
    env_index = torch.arange(E, device=DEV, dtype=torch.int32).repeat_interleave(P)
    s0, g0, _, _ = PG.sample_problems(gen, sdf, E * P, env_index=env_index, seed=WINDING_SEED, diagonal=torch.full((E * P,), -1, dtype=torch.int32, device=DEV))
    assert torch.equal(s0[..., :2], start[..., :2]) and torch.equal(g0[..., :2], goal[..., :2]) and torch.equal(s0[:, 0, 2], start[:, 0, 2])
    d = (goal[:, 0, 2] - g0[:, 0, 2]).cpu().numpy()
    full_turn = np.abs(np.abs(d) - HO.TWO_PI) < 1e-12
    print('goal headings a full turn from the straight line\'s: %d of %d' % (int(full_turn.sum()), d.size))
    assert (full_turn | (np.abs(d) < 1e-12)).all() and full_turn.any()
  ds = PlanningDataset(str(tmp_path), 'train')
  assert len(ds) == E * P
  for k in range(E * P):
    s = ds[k]
    assert np.array_equal(s['goal'].numpy(), goal[k].cpu().numpy()) and np.array_equal(s['start'].numpy(), start[k].cpu().numpy())
    assert s['goal'].numpy()[0, 2] == th_init[k, -1, 2].item()
