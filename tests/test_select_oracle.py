"""CPU-only tests of the multi-start selection (dgp_select_samples and what sits on top of it): the rule of include/dgpmp2_hip.h as tests/select_oracle.py restates
it -- coverage of the case set (tests/select_cases.py), the properties of the order -- the torch mirror utils.planner_utils.select_samples_torch against the
oracle, host-side argument validation of the entry point and dgp_select_launch_shape.  The kernel itself: tests/test_hip_select.py (-m gpu).

The base set is interp_cases.mixed_batch(dof, n, B S, (16,16), seed=3) reshaped to (B,S), for (B,S) in select_cases.BS and (n,K) in select_cases.NK; nearly every
trajectory of it that leaves the limits also collides, so select_cases.additions adds what separates require_inside from COLLIDING, the ties, the non-finite
scores and values and the excluded winner."""
import numpy as np
import pytest
import torch

import harness
import interp_cases as IC
import interp_oracle as IO_
import parity_cases as PC
import select_cases as SC
import select_oracle as SO
from dgpmp2_amd import _capi
from dgpmp2_amd.utils import planner_utils as PU

DOFS = (2, 3)


def oracle(c, K, **kw):
  return SO.run(c['p'], c['th'], K, c['sdf'], 0.0, c['score'], c['exclude'], **kw)


@pytest.fixture(scope='module')
def results():
  """the oracle on every case, computed once: {(dof, n, K, name): (case, Result)}"""
  out = {}
  for dof in DOFS:
    for n, K in SC.NK + (SC.NK32,):
      for name, c in SC.all_cases(dof, n):
        out[(dof, n, K, name)] = (c, oracle(c, K))
  return out


def test_case_set_covers_every_tier_tie_and_rejection(results):
  for dof in DOFS:
    for n, K in SC.NK:
      tiers, accepted = set(), {}
      for name, _ in SC.all_cases(dof, n):
        c, r = results[(dof, n, K, name)]
        tiers |= set(r.tier.ravel().tolist())
        accepted[name] = (r.tier == 0).sum(1)
      assert tiers == {0, 1, 2}, (dof, n, K)
      assert any((v == 0).any() for v in accepted.values())                                       # some problem has no accepted sample
      print('dof %d n %d K %d accepted per problem: %s' % (dof, n, K, {k: v.tolist() for k, v in accepted.items() if v.size <= 7}))
      # half of the base set's trajectories leave the limits, nearly all of those collide as well: the base set barely separates OUTSIDE from COLLIDING ...
      c, r = results[(dof, n, K, 'base B 2 S 70')]
      assert ((r.status & SO.OUTSIDE) != 0).sum() == 70
      # ... the additions do, on purpose: an end state alone outside the limits, the interior free
      c, r = results[(dof, n, K, 'additions')]
      assert r.status[0, 5] == SO.OUTSIDE and r.status[1, 5] == SO.OUTSIDE and r.status[2, 6] == SO.OUTSIDE
      d = IO_.dense(c['p'], c['th'][0, 5][None], K)[0]
      assert d[-1, 0] < -5.0 and (np.abs(d[:-1, 0]) <= 5.0).all()                                  # the END state alone
      assert r.order[0].tolist() == [3, 4, 1, 2, 0, 5, 6, 7] and r.tier[0].tolist() == [0, 0, 0, 0, 0, 1, 2, 2]
      assert r.status[0, 6] & SO.NON_FINITE and r.status[0, 7] == SO.EXCLUDED and r.score[0, 7] < r.score[0, 3]      # the excluded sample would have won
      assert np.signbit(c['score'][0, 4]) and not np.signbit(c['score'][0, 3])                   # the -0.0 / 0.0 pair ties in tier 0: the index decides
      assert (r.tier[1] >= 1).all() and r.problem_summary[1, SO.COL['solved']] == 0 and r.problem_summary[1, SO.COL['num_accepted']] == 0      # no accepted sample
      assert r.order[1].tolist()[:1] == [5] and r.max_pen[1, 0] == r.max_pen[1, 1] == r.max_pen[1, 2] == r.max_pen[1, 3] != r.max_pen[1, 4]
      pa, pb = r.max_pen[1, 0], r.max_pen[1, 4]
      assert r.order[1].tolist()[1:6] == ([2, 3, 0, 1, 4] if pa < pb else [4, 2, 3, 0, 1])         # ties inside tier 1: score -0.0 / 0.0, then 1.0 / 1.0, by index
      assert r.tier[1, 6] == 2 and r.tier[1, 7] == 2 and np.isnan(c['score'][1, 6]) and np.isinf(c['score'][1, 7])
      assert r.order[2].tolist()[:4] == [2, 7, 1, 4]
      # require_inside changes some best
      r2 = oracle(c, K, require_inside=False)
      assert r.best.tolist()[0] == 3 and r2.best.tolist()[0] == 5 and r2.tier[1, 5] == 0 and r2.problem_summary[1, SO.COL['solved']] == 1
      assert np.array_equal(r.status, r2.status)


def test_order_properties(results):
  for (dof, n, K, name), (c, r) in results.items():
    B, S = r.order.shape
    assert (np.sort(r.order, 1) == np.arange(S)).all(), name                                      # a permutation
    t = np.take_along_axis(r.tier, r.order, 1)
    assert (np.diff(t, axis=1) >= 0).all() and (r.best == r.order[:, 0]).all()                     # tiers never decrease along it
    assert IC.same_bits(r.th_best, c['th'][np.arange(B), r.best])
    assert np.array_equal(r.problem_summary[:, SO.COL['best_index']], r.best) and np.array_equal(r.problem_summary[:, SO.COL['best_status']], r.status[np.arange(B), r.best])


@pytest.mark.parametrize('dof', DOFS)
def test_best_follows_a_permutation_of_the_samples_and_the_layout_of_th(dof):
  n, K = 17, 2
  for B, S in ((3, 17), (7, 4)):
    c = SC.base(dof, n, B, S)
    r = oracle(c, K)
    assert len(set(c['score'].ravel().tolist())) == B * S                                          # distinct keys
    perm = np.random.RandomState(5).permutation(S)
    cp = dict(c, th=c['th'][:, perm], score=c['score'][:, perm], exclude=c['exclude'][:, perm])
    rp = oracle(cp, K)
    assert np.array_equal(perm[rp.best], r.best) and np.array_equal(perm[rp.order], r.order) and IC.same_bits(rp.th_best, r.th_best)
    sm = SO.run(c['p'], np.swapaxes(c['th'], 0, 1), K, c['sdf'], 0.0, c['score'].T, c['exclude'].T, sample_major=True)
    for k in ('status', 'tier', 'order', 'best', 'problem_summary', 'th_best', 'sample_summary'):
      assert IC.same_bits(getattr(sm, k), getattr(r, k)), k


def test_without_a_grid_nothing_collides_and_env_index_picks_the_grid():
  c = SC.additions(2, 17)
  r = SO.run(c['p'], c['th'], 2, None, 0.0, c['score'], c['exclude'])
  assert not (r.status & SO.COLLIDING).any() and r.sample_summary is None and not r.max_pen.any() and (r.status[0, 5] & SO.OUTSIDE)
  assert r.order[1].tolist() == [2, 3, 0, 1, 4, 5, 6, 7]                                          # scores decide tier 0; tier 1 is the start_out sample alone
  grids = SC.distinct_grids(c['sdf'], 5)
  env = np.array([4, 0, 2])
  a = SO.run(c['p'], c['th'], 2, grids, 0.0, c['score'], c['exclude'], env_index=env)
  b = SO.run(c['p'], c['th'], 2, grids[env], 0.0, c['score'], c['exclude'])
  assert IC.same_bits(a.sample_summary, b.sample_summary) and np.array_equal(a.order, b.order)
  assert not IC.same_bits(a.sample_summary, SO.run(c['p'], c['th'], 2, c['sdf'], 0.0, c['score'], c['exclude']).sample_summary)


@pytest.mark.parametrize('dof', DOFS)
def test_torch_mirror_equals_the_oracle(dof, results):
  AVG = IO_.COL['avg_penetration']
  for n, K in SC.NK:
    for name, _ in SC.all_cases(dof, n):
      c, r = results[(dof, n, K, name)]
      p = c['p']
      for require_inside, sample_major in ((True, False), (False, True)):
        want = r if require_inside else oracle(c, K, require_inside=False)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, 0, 1) if sample_major else a))
        th_best, info = PU.select_samples_torch(t(c['th']), torch.from_numpy(c['sdf']), t(c['score']), t(c['exclude']), total_time_sec=p.total_time_sec, x_lims=p.x_lims,
                                                y_lims=p.y_lims, sphere_radius=p.radius, num_inter=K, eps=0.0, require_inside=require_inside, sample_major=sample_major)
        tag = (dof, n, K, name, require_inside)
        assert np.array_equal(info.status.numpy(), want.status) and np.array_equal(info.order.numpy(), want.order) and np.array_equal(info.best.numpy(), want.best), tag
        assert IC.same_bits(th_best.numpy(), want.th_best), tag
        assert np.array_equal(info.solved.numpy(), want.problem_summary[:, 0] != 0) and np.array_equal(info.num_accepted.numpy(), want.problem_summary[:, 1]), tag
        assert np.array_equal(info.colliding.numpy(), (want.status & SO.COLLIDING) != 0) and np.array_equal(info.outside.numpy(), (want.status & SO.OUTSIDE) != 0)
        assert np.array_equal(info.non_finite.numpy(), (want.status & SO.NON_FINITE) != 0) and np.array_equal(info.excluded.numpy(), (want.status & SO.EXCLUDED) != 0)
        got, ws = info.sample_raw.numpy(), want.sample_summary
        assert np.array_equal(got[:, :, IO_.EXACT], ws[:, :, IO_.EXACT]), tag
        e = np.abs(got[:, :, AVG] - ws[:, :, AVG]) / np.maximum(np.abs(ws[:, :, AVG]), 1e-300)
        e[got[:, :, AVG] == ws[:, :, AVG]] = 0.0
        assert (e < PC.TOL_ERR['f64']).all(), (tag, e.max())
        raw = info.raw.numpy()
        assert np.array_equal(raw[:, [0, 1, 2, 5]], want.problem_summary[:, [0, 1, 2, 5]]) and IC.same_bits(raw[:, 3], want.problem_summary[:, 3]), tag


def _cfg(**kw):
  base = dict(num_states=64, dof=2, io_dtype=_capi.DGP_F32, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)
  base.update(kw)
  return _capi.make_config(**base)


def test_entry_point_validates_arguments_without_gpu():
  """every call below fails validation, so nothing is launched"""
  api = _capi.get_api()
  assert 'select_samples' in _capi.CApi.SYMBOLS and 'select_launch_shape' in _capi.CApi.SYMBOLS and api.select_samples is not None
  assert api.abi_version() == 7 == _capi.DGP_ABI_VERSION
  assert _capi.DGP_SELECT_COUNT == 6 and _capi.SELECT_NAMES == SO.NAMES == PU.SELECT_NAMES
  assert (_capi.DGP_SEL_COLLIDING, _capi.DGP_SEL_OUTSIDE, _capi.DGP_SEL_NON_FINITE, _capi.DGP_SEL_EXCLUDED) == (SO.COLLIDING, SO.OUTSIDE, SO.NON_FINITE, SO.EXCLUDED) == (1, 2, 4, 8)
  import ctypes as C
  assert C.sizeof(_capi.DgpSelectParams) == 24
  s = _capi.Solver(_cfg())
  ok, P = s.sdf_arg(0x1000, 256, 256, 0), s.select_params

  def bad(word, *a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      s.select_samples(*a, **kw)
    assert e.value.code == _capi.DGP_EINVAL and word in str(e.value), (word, str(e.value))
  bad('batch', 0, 4, 0x1000, P(), best=0x1000)
  bad('batch', -2, 4, 0x1000, P(), best=0x1000)
  bad('num_samples', 8, 0, 0x1000, P(), best=0x1000)
  bad('num_samples', 8, 1025, 0x1000, P(), best=0x1000)
  bad('batch * num_samples', 1 << 22, 1 << 9, 0x1000, P(), best=0x1000)
  bad('num_inter', 8, 4, 0x1000, P(num_inter=-1), best=0x1000)
  bad('num_inter', 8, 4, 0x1000, P(num_inter=1024), best=0x1000)
  bad('eps', 8, 4, 0x1000, P(eps=float('nan')), best=0x1000)
  bad('eps', 8, 4, 0x1000, P(eps=float('inf')), best=0x1000)
  bad('th', 8, 4, None, P(), best=0x1000)
  bad('DgpSelectParams', 8, 4, 0x1000, None, best=0x1000)
  wrong = P()
  wrong.struct_size = 20
  bad('struct_size', 8, 4, 0x1000, wrong, best=0x1000)
  bad('all null', 8, 4, 0x1000, P(), sdf=ok)
  bad('sample_summary', 8, 4, 0x1000, P(), sample_summary=0x1000)
  bad('sample_summary', 8, 4, 0x1000, P(), sdf=s.sdf_arg(None, 256, 256, 0), sample_summary=0x1000)
  bad('env_index', 8, 4, 0x1000, P(), env_index=0x1000, best=0x1000)
  assert api.select_samples(None, 8, 4, 0x1000, None, None, None, None, C.byref(P()), None, 0x1000, None, None, None, None, None) == _capi.DGP_EINVAL
  assert b'handle' in api.last_error()
  s2 = _capi.Solver(_cfg(num_states=2))
  with pytest.raises(_capi.DgpError) as e:                                                         # n = 2, K = 0 with a grid: two dense states, no interior one
    s2.select_samples(8, 4, 0x1000, P(num_inter=0), sdf=ok, best=0x1000)
  assert e.value.code == _capi.DGP_EINVAL and 'interior' in str(e.value) and 'num_inter' in str(e.value)
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  bad('batch', 0, 4, 0x1000, P(), best=0x1000)
  assert api.time_next_launch(None, None) == _capi.DGP_OK


def test_launch_shape():
  for (n, K), lpt in SC.LPT.items():
    s = _capi.Solver(_cfg(num_states=n))
    assert IO_.lpt(IO_.num_dense(n, K)) == lpt
    for S in (1, 3, 4, 17, 70, 1024):
      l, w, ps = s.select_launch_shape(S, K)
      tpw = 64 // lpt
      assert l == lpt and 1 <= w <= 16 and w == min(16, -(-S // tpw)) and ps == -(-S // (w * tpw)) and w * tpw * ps >= S, (n, K, S, l, w, ps)
  s = _capi.Solver(_cfg(num_states=33))
  assert s.select_launch_shape(70, 7) == (64, 16, 5) and s.select_launch_shape(17, 7) == (64, 16, 2)      # LPT 64: 70 samples in more than one pass, 17 on more than one wavefront
  assert _capi.Solver(_cfg(num_states=17)).select_launch_shape(17, 2) == (16, 5, 1)
  for a in ((0, 7), (1025, 7), (8, -1), (8, 1024)):
    with pytest.raises(_capi.DgpError):
      s.select_launch_shape(*a)


def test_emulator_library_reports_the_entry_point_as_absent():
  api = harness.emul_api()
  assert api.select_samples is None and api.select_launch_shape is None
  s = _capi.Solver(_cfg(), api=api)
  with pytest.raises(NotImplementedError, match='emul_select_samples'):
    s.select_samples(8, 4, 0x1000, s.select_params(), best=0x1000)
