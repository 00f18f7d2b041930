"""dgp_step_loss / dgp_step_loss_backward on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through the planner.

  * forward against tests/loss_oracle.py: the gp / sg / obs columns of per_traj bit for bit; the pos / vel rows and the batch terms within (N + 8) 2^-53 relative, N the
    number of addends (identical bits in kernel and oracle, all non-negative: any summation order stays within (N - 1) 2^-53; the 8 covers the divisions and the
    weighted combinations; EXT and TOTAL: N the largest of their parts); against fixture g12_step_loss (the reference's own text) at twice that, gradients at 8 x 2^-53;
  * backward against the oracle: every gradient bit for bit, fp64 and fp32, each output alone;
  * shapes: n in {1, 2, 3, 17, 65, 130, 257} (all three lanes-per-trajectory instantiations, asserted) x B in {1, 5, 63, 64, 65, 67, 1025} (ragged wavefronts, a ragged
    second-stage reduction), dof 2 and 3, one call at B = 4096, n = 64; tests/loss_cases.mixed_batch puts exact hits, large and ordinary trajectories side by side;
  * call forms (three-array against two-array, absent errors, every buffer off the 16-byte boundary under guard bands), determinism (two runs, two batch positions,
    two batch sizes), a planted NaN, the sign of a zero gradient;
  * through the planner: tests/tbptt_driver.truncated_bptt with the device loss on fixture g7_tbptt, and a graphed iteration replayed against the eager call."""
import numpy as np
import pytest
import torch

import harness
import loss_cases as LC
import loss_oracle as LO
from dgpmp2_amd import _capi
from test_loss_oracle import GRAD_TOL, fixture_cases, grads_close, terms_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NS, BS = (1, 2, 3, 17, 65, 130, 257), (1, 5, 63, 64, 65, 67, 1025)
W = LC.WEIGHTS[0]
GRADS = ('update', 'target', 'target_sub', 'sg', 'gp', 'obs')


@pytest.fixture(scope='module')
def be():
  b = harness.Backend('hip')
  yield b
  b.guard = b.misalign = False


def _code(io): return _capi.DGP_F64 if io == 'f64' else _capi.DGP_F32


def fwd(be, c, w, dof, io, sub=True, errs=('sg', 'gp', 'obs')):
  """dgp_step_loss -> terms (8,), per_traj (B, 5)"""
  be._keep, be._rec = [], {}
  B, n, _ = c['update'].shape
  p = {k: be.to_dev(c[k], io, name=k)[1] for k in ('update', 'target')}
  p['target_sub'] = be.to_dev(c['target_sub'], io, name='target_sub')[1] if sub else None
  for k in ('sg', 'gp', 'obs'): p[k] = be.to_dev(c[k], io, name='unw_' + k)[1] if k in errs else None
  terms, terms_p = be.empty((_capi.DGP_LOSS_COUNT,), dtype=np.float64, name='terms')
  per, per_p = be.empty((B, _capi.DGP_LOSS_PER_TRAJ), dtype=np.float64, name='per_traj')
  _capi.step_loss(_code(io), B, n, dof, p['update'], p['target'], w, terms_p, per_p, target_sub=p['target_sub'], unw_sg=p['sg'], unw_gp=p['gp'], unw_obs=p['obs'],
                  stream=be.stream())
  out = be.to_np(terms), be.to_np(per)
  be._done()
  return out


def bwd(be, c, w, dof, io, g=None, sub=True, want=GRADS):
  """dgp_step_loss_backward -> dict of the gradients asked for (float64 copies), None for the others"""
  be._keep, be._rec = [], {}
  B, n, d = c['update'].shape
  p = {k: be.to_dev(c[k], io, name=k)[1] for k in ('update', 'target')}
  p['target_sub'] = be.to_dev(c['target_sub'], io, name='target_sub')[1] if sub else None
  g_p = None if g is None else be.to_dev(np.array([g]), dtype=np.float64, name='g_total')[1]
  bufs = {k: (be.empty((B, n, d) if k in GRADS[:3] else (B,), io, name='g_' + k) if k in want else (None, None)) for k in GRADS}
  _capi.step_loss_backward(_code(io), B, n, dof, p['update'], p['target'], w, target_sub=p['target_sub'], g_total=g_p, g_update=bufs['update'][1],
                           g_target=bufs['target'][1], g_target_sub=bufs['target_sub'][1], g_unw_sg=bufs['sg'][1], g_unw_gp=bufs['gp'][1], g_unw_obs=bufs['obs'][1],
                           stream=be.stream())
  out = {k: be.to_np(bufs[k][0]) for k in GRADS}
  be._done()
  return out


def check_forward(tag, got, c, w, dof):
  """-> list of failure strings"""
  terms, per = got
  B, n, _ = c['update'].shape
  want_t, want_p = LO.forward(c['update'], c['target'], c['target_sub'], c['sg'], c['gp'], c['obs'], w, dof)
  bad = []
  if not LC.same_bits(per[:, 2:], want_p[:, 2:]): bad.append('%s: the gp / sg / obs columns of per_traj are not the inputs' % tag)
  e = np.abs(per[:, :2] - want_p[:, :2]) / np.maximum(np.abs(want_p[:, :2]), 1e-300)
  e[per[:, :2] == want_p[:, :2]] = 0.0
  if not (e <= LO.sum_bound(n * dof)).all(): bad.append('%s: pos / vel rows at %.3g of the bound' % (tag, e.max() / LO.sum_bound(n * dof)))
  ok, frac = terms_close(terms, want_t, B, n, dof=dof)
  if not ok: bad.append('%s: terms at %s of the bound' % (tag, np.round(frac, 3).tolist()))
  return bad


def check_backward(tag, got, c, w, dof, io, g, sub=True):
  want = LO.backward(c['update'], c['target'], c['target_sub'] if sub else None, w, dof, g=1.0 if g is None else g, io=io)
  return ['%s: g_%s differs from the oracle in %d entries' % (tag, k, int((LC.bits(got[k]) != LC.bits(want[k])).sum())) for k in GRADS
          if got[k] is not None and not LC.same_bits(got[k], want[k])]


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('dof', [2, 3])
def test_every_shape_against_the_oracle(be, dof, io):
  bad, lpts = [], set()
  full = {3: 16, 17: 32, 65: 64}      # n run with every batch size, one per lanes-per-trajectory count
  for i, n in enumerate(NS):
    lpts.add(LO.lpt(n))
    if n in full: assert LO.lpt(n) == full[n]
    for B in (BS if n in full else (BS[(i + dof) % len(BS)],)):
      c = LC.mixed_batch(dof, n, B, seed=n)
      w = LC.WEIGHTS[(n + B) % 2]
      g = None if (n + B) % 3 == 0 else 0.7
      tag = 'dof %d %s n %d B %d' % (dof, io, n, B)
      bad += check_forward(tag, fwd(be, c, w, dof, io), c, w, dof)
      bad += check_backward(tag, bwd(be, c, w, dof, io, g), c, w, dof, io, g)
  assert lpts == {16, 32, 64}
  assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_the_benchmark_shape(be, io):
  c = LC.mixed_batch(2, 64, 4096)
  assert not check_forward('B 4096 n 64 ' + io, fwd(be, c, W, 2, io), c, W, 2)
  assert not check_backward('B 4096 n 64 ' + io, bwd(be, c, W, 2, io, 0.7), c, W, 2, io, 0.7)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_against_the_reference_fixture(be, golden, io):
  g = golden('g12_step_loss')
  cot = float(g['cotangent'])
  for B, n, c, w, ref in fixture_cases(g):
    terms, per = fwd(be, c, w, 2, io)
    ok, frac = terms_close(terms, ref['terms'], B, n, factor=2.0)
    assert ok, (B, n, w, frac)
    gr = bwd(be, c, w, 2, io, cot)
    tol = GRAD_TOL if io == 'f64' else 2.0 ** -24 + GRAD_TOL      # fp32 I/O: the one rounding of the stored value
    for mine, theirs in (('update', 'g_update'), ('target_sub', 'g_target_sub'), ('sg', 'g_sg'), ('gp', 'g_gp'), ('obs', 'g_obs')):
      assert grads_close(gr[mine], ref[theirs], tol), (B, n, w, mine)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_each_output_alone_and_call_forms(be, io):
  for dof, n, B in ((2, 17, 67), (3, 3, 65), (2, 130, 5)):
    c = LC.mixed_batch(dof, n, B, seed=2)
    ref_f, ref_b = fwd(be, c, W, dof, io), bwd(be, c, W, dof, io, 0.7)
    tag = (dof, n, B, io)
    # two runs: the same bits
    again_f, again_b = fwd(be, c, W, dof, io), bwd(be, c, W, dof, io, 0.7)
    assert LC.same_bits(again_f[0], ref_f[0]) and LC.same_bits(again_f[1], ref_f[1]) and all(LC.same_bits(again_b[k], ref_b[k]) for k in GRADS), tag
    # each gradient alone, and PlanLayer's patterns: the present ones bit-equal, the absent ones not written (they are NULL)
    for want in [(k,) for k in GRADS] + [('update', 'sg', 'gp', 'obs'), ('update', 'target_sub')]:
      only = bwd(be, c, W, dof, io, 0.7, want=want)
      assert all((only[k] is None) == (k not in want) for k in GRADS) and all(LC.same_bits(only[k], ref_b[k]) for k in want), (tag, want)
    # the three-array form against the two-array form on the pre-formed difference (exact for these inputs; formed in fp64 on the host)
    two = dict(c, target=c['target'] - c['target_sub'])
    two_f, two_b = fwd(be, two, W, dof, io, sub=False), bwd(be, two, W, dof, io, 0.7, sub=False, want=('update', 'target', 'target_sub', 'sg'))
    assert LC.same_bits(two_f[0], ref_f[0]) and LC.same_bits(two_f[1], ref_f[1]), tag
    assert all(LC.same_bits(two_b[k], ref_b[k]) for k in ('update', 'target', 'target_sub', 'sg')), tag      # (g_target_sub without target_sub: m k)
    # absent errors: the term is 0
    for errs in ((), ('gp',), ('sg', 'obs')):
      zeroed = dict(c, **{k: np.zeros(B) for k in ('sg', 'gp', 'obs') if k not in errs})
      got, want = fwd(be, c, W, dof, io, errs=errs), fwd(be, zeroed, W, dof, io)
      assert LC.same_bits(got[0], want[0]) and LC.same_bits(got[1], want[1]), (tag, errs)
      assert all(got[0][LO.COL[k]] == 0.0 for k in ('sg', 'gp', 'obs') if k not in errs)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_unaligned_buffers_give_the_same_bits(be, io):
  """every buffer one element off the 16-byte boundary, inputs only, outputs only -- under guard bands: no store outside an output, no store into an input"""
  for dof, n, B in ((2, 17, 67), (3, 3, 65), (3, 65, 5), (2, 257, 3)):
    c = LC.mixed_batch(dof, n, B, seed=4)
    ref_f, ref_b = fwd(be, c, W, dof, io), bwd(be, c, W, dof, io, 0.7)
    be.guard = True
    try:
      checks = be.guard_checks
      for mis in (False, True, 'inputs', 'outputs'):
        be.misalign = mis
        got_f, got_b = fwd(be, c, W, dof, io), bwd(be, c, W, dof, io, 0.7)
        assert LC.same_bits(got_f[0], ref_f[0]) and LC.same_bits(got_f[1], ref_f[1]), (dof, n, B, io, mis)
        assert all(LC.same_bits(got_b[k], ref_b[k]) for k in GRADS), (dof, n, B, io, mis)
      assert be.guard_checks > checks + 4 * 8
    finally:
      be.guard = be.misalign = False


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_rows_do_not_depend_on_batch_position_or_size(be, io):
  for dof, n, B in ((2, 17, 67), (3, 65, 65), (2, 3, 1025)):
    c = LC.mixed_batch(dof, n, B, seed=6)
    ref = fwd(be, c, W, dof, io)[1]
    rolled = fwd(be, {k: np.roll(v, 1, 0) for k, v in c.items()}, W, dof, io)[1]
    assert LC.same_bits(rolled, np.roll(ref, 1, 0)), (dof, n, B, io)
    head = fwd(be, {k: v[:5] for k, v in c.items()}, W, dof, io)[1]
    assert LC.same_bits(head, ref[:5]), (dof, n, B, io)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_nan_and_signed_zero(be, io):
  dof, n, B = 2, 17, 67
  c = LC.mixed_batch(dof, n, B, seed=8)
  c['update'][9, 11, 3] = np.nan
  terms, per = fwd(be, c, W, dof, io)
  assert np.isnan(per[9, 1]) and not np.isnan(np.delete(per, 9, 0)).any() and not np.isnan(per[9, [0, 2, 3, 4]]).any()      # that row's velocity sum, nothing else
  assert np.isnan(terms[LO.COL['vel']]) and np.isnan(terms[LO.COL['total']]) and not np.isnan(terms[[LO.COL[k] for k in ('pos', 'cov', 'gp', 'sg', 'obs', 'ext')]]).any()
  gr = bwd(be, c, W, dof, io, 0.7)
  assert np.isnan(gr['update'][9, 11, 3]) and np.isnan(gr['update']).sum() == 1
  assert not check_backward('nan', gr, c, W, dof, io, 0.7)
  # a miss of exactly 0 (trajectories 0, 4, ...): +0.0 for update and target_sub, -0.0 for target, as the oracle says; with a negative cotangent the other way round
  for g in (0.7, -0.7):
    gr = bwd(be, c, W, dof, io, g)
    assert not check_backward('zero', gr, c, W, dof, io, g)
    assert not gr['update'][0].any() and bool(np.signbit(gr['update'][0]).all()) == (g < 0) and bool(np.signbit(gr['target'][0]).all()) == (g > 0)


@pytest.mark.parametrize('fused', [False, True], ids=['step+errors', 'step_with_errors'])
@pytest.mark.parametrize('tag,mode,mtype', [('fix_dynamics', 'fix_dynamics', 'feed_forward'), ('qc_full', 'qc_full', 'feed_forward'), ('recurrent', 'fix_dynamics', 'recurrent')])
def test_through_the_planner_tbptt(golden, tag, mode, mtype, fused):
  """tests/tbptt_driver.truncated_bptt with the device loss in place of its torch loss: the assertions and bounds of test_planner_api.test_tbptt_outer_loop_runs"""
  import copy
  import tbptt_driver as TD
  import test_planner_api as TPA
  from conftest import rel_err
  from dgpmp2_amd.gpmp2 import plan_layer as PL
  from dgpmp2_amd.utils.planner_utils import straight_line_trajb
  from oracle import gpmp2_oracle as O
  pc = _capi.get_pycall()
  calls = []

  def device_loss(update, expert_update, e_sg, e_gp, e_obs, weights):      # the driver's loss_fn call: the two-array form
    calls.append(1)
    return PL.device_step_loss(pc, 2, update, expert_update, None, (e_sg, e_gp, e_obs), weights)
  g = golden('g7_tbptt')
  B, n, G = 3, 16, int(g['G'])
  T = TPA.T
  lp = copy.deepcopy(TPA.TBPTT_LEARN_PARAMS)
  lp['dgpmp2']['dynamics_mode'] = mode
  lp['model']['type'] = mtype
  planner, pp = TPA._learn_planner(n, B, lp)
  dg = lp['dgpmp2']
  sdf = T(O.circles_sdf(G, g['circles']))[None, None].repeat(B, 1, 1, 1)
  batch = {'im': (sdf > 0).double(), 'sdf': sdf.clone().requires_grad_(True), 'start': T(g['start']), 'goal': T(g['goal']), 'th_opt': T(g['th_opt'])}
  th_init = straight_line_trajb(batch['start'][:, :, :2], batch['goal'][:, :, :2], pp['total_time_sec'], pp['total_time_step'], 2, torch.device(DEV))
  th_init.requires_grad_(True)
  r = TD.truncated_bptt(planner, batch, th_init, dg['T'], dg['tk'], dg['tk2'], lp['optim'], recurrent=(mtype == 'recurrent'), loss_fn=device_loss, fused=fused)
  pre, what = tag + '_', (tag, fused)
  ref_terms = g[pre + 'terms']
  mine = np.asarray([[float(x.detach()) for x in (t.total, t.pos, t.vel, t.cov, t.gp, t.sg, t.obs, t.ext)] for t in r['terms']])
  assert mine.shape == ref_terms.shape, what
  for col, name in enumerate(LO.NAMES):
    assert rel_err(mine[:, col], ref_terms[:, col]) < 1e-9 or float(np.abs(ref_terms[:, col]).max()) == 0.0, (what, name)
  grads = {name: p.grad for name, p in planner.named_parameters()}
  assert sorted(grads.keys()) == list(g[pre + 'param_names']), what
  assert rel_err(r['th_final'].cpu().numpy(), g[pre + 'th_final']) < 1e-9, what
  assert rel_err(r['err'].cpu().numpy(), g[pre + 'err']) < 1e-9 and rel_err(r['err_ext'].cpu().numpy(), g[pre + 'err_ext']) < 1e-9, what
  for name, gr in grads.items():
    assert rel_err(gr.cpu().numpy(), g[pre + 'grad_' + name.replace('.', '_')]) < 1e-8, (what, name)
  assert rel_err(batch['sdf'].grad.cpu().numpy(), g[pre + 'sdf_grad']) < 1e-8, what
  assert rel_err(r['last_input_leaf'].grad.cpu().numpy(), g[pre + 'th_curr_grad_last']) < 1e-8, what
  assert (th_init.grad is None) == bool(g[pre + 'th_init_grad_is_none']), what
  assert len(calls) == dg['T']


def _planner(n, B):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_graphed_iteration_replays_the_eager_call(dtype):
  """step_with_errors + step_loss + backward as one graphed iteration, replayed three times with fresh inputs: bit-identical to the eager call; and the planner's loss
  against the oracle on what the step produced"""
  from oracle import gpmp2_oracle as O
  n, B, G = 17, 67, 32
  planner = _planner(n, B)
  weights = dict(vel_loss_lambda=0.5, ext_obs_lambda=2.0, ext_loss_weight=0.3)
  sdf = torch.from_numpy(O.circles_sdf(G, O.C2_CIRCLES)).to(dtype).to(DEV)[None, None].expand(B, 1, G, G)

  def inputs(seed):
    rs = np.random.RandomState(seed)
    start, goal = np.zeros((B, 1, 4)), np.zeros((B, 1, 4))
    start[:, 0, :2], goal[:, 0, :2] = rs.uniform(-4, 4, (B, 2)), rs.uniform(-4, 4, (B, 2))
    th = O.straight_line_trajb(start[:, :, :2], goal[:, :, :2], 10.0, n - 1, 2) + rs.randn(B, n, 4) * 0.05
    th_opt = th + rs.randn(B, n, 4) * 0.3
    to = lambda a: torch.from_numpy(a).to(dtype).to(DEV)
    return to(th).requires_grad_(True), to(start), to(goal), to(th_opt)

  def iteration(th, start, goal, th_opt):
    out, errors = planner.step_with_errors(th, start, goal, None, sdf)
    loss = planner.step_loss(out[0], th, th_opt, errors, weights)
    g_th, = torch.autograd.grad(loss.total, th)
    return loss.raw, loss.per_sample, g_th, out[0], errors[0], errors[1], errors[2]
  it = planner.graphed_iteration(iteration, clone_outputs=True)
  for seed in (1, 2, 3):
    args = inputs(seed)
    eager = [t.detach().clone() for t in iteration(*args)]
    replay = it(*args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(replay, eager)), seed
    assert it.captures == 1
    # the loss of the planner against the oracle, on the update and the errors the step produced
    raw, per, g_th, dth, e_sg, e_gp, e_obs = (t.double().cpu().numpy() for t in eager)
    c = dict(update=dth, target=args[3].detach().double().cpu().numpy(), target_sub=args[0].detach().double().cpu().numpy(), sg=e_sg.reshape(B), gp=e_gp.reshape(B), obs=e_obs.reshape(B))
    w = (0.5, 2.0, 0.3)
    assert not check_forward('planner seed %d' % seed, (raw, per), c, w, 2)
    assert np.isfinite(g_th).all() and np.abs(g_th).max() > 0
