"""CPU: the lane-mixed batches of tests/lane_mix.py and the checks of tests/test_hip_full_batch.py, before they reach a GPU.
  * coverage -- every configuration the GPU test runs has, in EVERY wavefront, a trajectory whose lanes take both sides of the
    hinge, states outside the grid, (C > 1) a lane with both sides inside its C states, (velocity limits) states on both sides of
    the limit; and the K = 3 stopping rule gives two or more iteration counts in >= 90 % of the wavefronts (C oracle; not for the
    step-only 'scalar' modes); every static configuration launches lane_mix.expected_variant's kernel variant (emulator), and each robot
    reaches block elimination with C = 4 and with C < 4 and both Woodbury variants;
  * sensitivity -- each planted fault (a host-side edit of a correct result) is reported by the checks;
  * pipeline -- the whole GPU test body on the CPU wavefront emulator at 3 wavefronts, one configuration per kernel family."""
import os
import numpy as np
import pytest
import harness
import parity_cases as PC
from dgpmp2_amd import _capi
import lane_mix as LM
from oracle import blocktri as BT

NTHREADS = max(1, min(16, os.cpu_count() or 1))


def _valid(bt):
  """(B, n) bool: the non-NaN trajectories' states"""
  return np.broadcast_to(LM.ok_rows(bt)[:, None], (bt.B, bt.n))


@pytest.mark.parametrize('dof', [2, 3])
def test_lane_mix_coverage(dof, monkeypatch):
  bad = []
  reached = set()
  for (lpt, c, n, cov, vel), grid in [(cf, None) for cf in LM.configs(dof)] + [(LM.odd_config(dof), LM.ODD_GRID)]:
    if grid is None: bt = LM.make(dof, lpt, c, n, cov, vel=vel, waves=LM.config_waves(cov), seed=1000 * dof + 10 * lpt + c)
    else: bt = LM.make(dof, lpt, c, n, cov, vel=vel, waves=LM.MIN_WAVES, seed=1000 * dof + 10 * lpt + c + 5, grid=grid)
    want_v = LM.expected_variant(lpt, c, n, cov, vel)
    if want_v is not None:      # the variant the same host dispatch picks under the forced shape
      monkeypatch.setenv('DGP_FORCE_SHAPE', '%d,%d' % (lpt, c))
      got = _capi.Solver(harness.config_from_oracle(bt.p, 'f64'), api=harness.emul_api()).step_kernel_variant(bt.B)
      if got != want_v: bad.append('%s: static kernel variant %d, expected %d' % (bt.tag, got, want_v))
      reached.add((got, c == 4) if got == 1 else got)
    T = LM.tpw(lpt)
    W = bt.waves + (T > 1)
    wave = np.arange(bt.B) // T
    act = LM.hinge_active(bt.p, bt.sdf, bt.th_clean, bt.eps)
    lanes = act.reshape(bt.B, -1)
    mixed_traj = lanes.any(1) & ~lanes.all(1)
    oog = LM.out_of_grid(bt.p, bt.sdf, bt.th_clean[:, :, :2]).any(1)
    for name, per_traj in (('mixed hinge lanes', mixed_traj), ('out-of-grid states', oog)):
      has = np.bincount(wave[per_traj], minlength=W) > 0
      if not has.all(): bad.append('%s: %d wavefronts without %s' % (bt.tag, (~has).sum(), name))
    if c > 1:
      full = (n // c) * c
      blk = act[:, :full].reshape(bt.B, -1, c)
      lane_mixed = (blk.any(2) & ~blk.all(2)).any(1)
      has = np.bincount(wave[lane_mixed], minlength=W) > 0
      if not has.all(): bad.append('%s: %d wavefronts without a lane of mixed hinge states' % (bt.tag, (~has).sum()))
    if vel:
      v = np.abs(bt.th_clean[:, :, dof:dof + 2]) >= 1.0
      both = v.reshape(bt.B, -1).any(1) & ~v.reshape(bt.B, -1).all(1)
      if not (np.bincount(wave[both], minlength=W) > 0).all(): bad.append('%s: wavefronts without mixed velocity limits' % bt.tag)
    if T >= 2 and not LM.is_scalar(cov):      # the K = 3 stopping rule at tol_delta = median first-step norm: two or more iteration counts per wavefront
      ok = LM.ok_rows(bt)
      d0 = BT.gn_step(bt.p, bt.th, bt.start, bt.goal, bt.sdf, nthreads=NTHREADS, **LM.okw(bt))[0]
      tol = LM.median_tol(d0[ok])
      _, its, _ = LM.stopping(bt, LM.okw(bt), tol, 3, NTHREADS, 0.0)
      nd = np.array([len(set(its[(wave == w) & ok].tolist())) for w in range(W)])
      if not (nd >= 2).mean() >= 0.9: bad.append('%s: only %.1f %% of wavefronts with two iteration counts' % (bt.tag, 100 * (nd >= 2).mean()))
  missing = {(1, True), (1, False), 3, 4} - reached
  if missing: bad.append('dof %d: static kernel variants never reached: %s' % (dof, sorted(map(str, missing))))
  assert not bad, '\n'.join(bad)


# ---- planted faults: host-side edits of correct results, each must be reported --------------------------------------------------------
@pytest.fixture(scope='module')
def small():
  bt = LM.make(2, 16, 4, 64, 'perstate', vel=True, waves=6, seed=5)
  d, e, x, i = BT.gn_step(bt.p, bt.th, bt.start, bt.goal, bt.sdf, nthreads=NTHREADS, **LM.okw(bt))
  return bt, d, e, x


def test_planted_stale_slot(small):
  """one lane's C rows of one trajectory in a middle wavefront replaced by the same lane's rows of the previous wavefront"""
  bt, d, _, _ = small
  T, c = LM.tpw(bt.lpt), bt.c
  b = 2 * T + 1; lane = 5
  got = d.copy(); got[b, lane * c:(lane + 1) * c] = d[b - T, lane * c:(lane + 1) * c]
  assert not LM.check_close(bt, 'step dtheta', d, d, PC.TOL['f64'])
  msg = LM.check_close(bt, 'step dtheta', got, d, PC.TOL['f64'])
  assert msg and 'wavefront 2, lane offset 16' in msg[0], msg
  # ... and by the rotation check, when the rotated run reads the other wavefront's slot
  r = T // 2 + 1
  assert LM.check_bit_equal(bt, 'step dtheta', d, np.roll(got, r, 0), r)


def _grads(bt, idx):
  from oracle import autograd_torch as AT
  rs = np.random.RandomState(3)
  sub = lambda a: None if a is None else a[idx]
  gbar = rs.randn(len(idx), bt.n, 2 * bt.dof); gext = rs.randn(len(idx))
  g = AT.step_gradients(bt.p, bt.th_clean[idx], bt.start[idx], bt.goal[idx], bt.sdf, gbar, gext, qc=sub(LM.oracle_qc(bt)), ow=sub(bt.ow), eps=sub(bt.eps), q_full=bt.q_full)
  return g, gbar, gext


def _subbatch(bt, idx):
  s = LM.Batch(); s.__dict__.update(bt.__dict__)
  for k in ('th', 'th_clean', 'start', 'goal', 'qc', 'ow', 'eps', 'qc_dense', 'raw_out'):
    a = getattr(bt, k); setattr(s, k, None if a is None else a[idx])
  s.th = s.th_clean      # (the NaN trajectory too, without its NaN)
  s.B = len(idx); s.nan_rows = np.zeros(0, np.int64)
  return s


@pytest.mark.parametrize('cfg', [(2, 16, 4, 64, 'perstate', True), (2, 64, 4, 256, 'static', True), (3, 64, 1, 61, 'perstate', False), (2, 64, 1, 64, 'qfull', False)],
                         ids=lambda c: 'dof%d_%d_%d_n%d_%s' % c[:5])
@pytest.mark.parametrize('rel', [0.03, 1e-3])
def test_planted_gradient_lane_error(cfg, rel):
  """a 3 % (and a 1e-3) relative error in one lane's rows of g_th -- in the lane the lane-resolved directional check probes in that trajectory -- against
  the extended-precision C oracle, in a short shape, an n = 256 shape and two one-trajectory-per-wavefront (LPT = 64) shapes.  Measured here with the
  autograd oracle's gradients: 7e-8 at worst on the correct ones (FD_LANE_TOL = 1e-4), 1e-3 on the planted lane."""
  dof, lpt, c, n, cov, vel = cfg
  bt = LM.make(dof, lpt, c, n, cov, vel=vel, waves=6, seed=5)
  idx = np.array([0, 1, 3, 5]) * LM.tpw(lpt)
  s = _subbatch(bt, idx)
  g, gbar, gext = _grads(bt, idx)
  grads = {k: g[k].reshape(getattr(s, k).shape) for k in ('th', 'start', 'goal', 'qc', 'ow', 'eps') if getattr(s, k) is not None}
  v = LM.direction(s); vl = LM.lane_direction(s, grads['th'])
  err, excl = LM.directional(s, grads, gbar, gext, v, nthreads=NTHREADS)
  errl, excll = LM.directional(s, grads, gbar, gext, vl, nthreads=NTHREADS)
  assert not excl.any() and not excll.any() and err.max() < LM.FD_TOL and errl.max() < LM.FD_LANE_TOL, (err, errl)      # the correct gradients pass
  lane = LM.probe_lane(s, 2)
  grads['th'] = grads['th'].copy(); grads['th'][2, lane * c:(lane + 1) * c] *= 1 + rel
  errl2, _ = LM.directional(s, grads, gbar, gext, vl, nthreads=NTHREADS)
  assert errl2[2] > 5 * LM.FD_LANE_TOL and (np.delete(errl2, 2) < LM.FD_LANE_TOL).all(), errl2      # (flagged with a factor 5 to spare)


def test_planted_fp32_row_error(small):
  """a 1e-4 relative error in one fp32 dtheta row: the fp32 / fp64 sibling check"""
  bt, d, _, _ = small
  d32 = PC.rnd(d, 'f32')
  assert not LM.check_close(bt, 'sibling step dtheta', d32, d, 1e-6)
  b, row = 9, 17
  got = d32.copy(); got[b, row] = PC.rnd(d32[b, row] * (1 + 1e-4), 'f32')
  msg = LM.check_close(bt, 'sibling step dtheta', got, d, 1e-6)
  assert msg and 'trajectory %d ' % b in msg[0], msg


def test_planted_nan_leak(small):
  """a NaN leaking from the NaN trajectory into a wave neighbour"""
  bt, d, _, _ = small
  clean = BT.gn_step(bt.p, bt.th_clean, bt.start, bt.goal, bt.sdf, nthreads=NTHREADS, **LM.okw(bt))[0]
  assert not LM.check_nan_isolation(bt, 'step dtheta', d, clean)
  b = int(bt.nan_rows[0])
  got = d.copy(); got[b + 1, 3, 0] = np.nan
  msg = LM.check_nan_isolation(bt, 'step dtheta', got, clean)
  assert msg and 'trajectory %d ' % (b + 1) in msg[0], msg


def _round5(bt, a):
  """the round-5 signature (profiles/r06_compiler_fault.md): row 0 of every lane >= 1 of EVERY trajectory off by 1e-3 -- wherever the trajectory sits"""
  a = a.copy()
  for j in range(1, -(-bt.n // bt.c)): a[:, j * bt.c] *= 1 + 1e-3
  return a


@pytest.mark.parametrize('what', ['step_errors dtheta', 'tiled backward g_th'])
def test_planted_round5_signature(small, what):
  """the same error in every trajectory: the new reference checks of the twins report it (naming a wavefront and a lane offset), the rotation check
  cannot -- the gap the per-trajectory references close"""
  bt, d, _, _ = small
  ok = LM.ok_rows(bt)
  if what == 'step_errors dtheta':
    ref = PC.rnd(d, 'f32')
    check = lambda got: LM.check_close(bt, '[f32] step_errors dtheta vs step', got, ref, LM.TWIN_STEP_TOL['f32'])
  else:
    idx = np.arange(bt.B)
    g, _, _ = _grads(bt, idx)
    ref = PC.rnd(g['th'].reshape(bt.th.shape), 'f32')
    check = lambda got: LM.check_grads(bt, '[f32] [tiled] backward vs row-major', dict(th=got), dict(th=ref), LM.TILED_GRAD_TOL['f32'], ok)
  assert not check(ref)
  got = _round5(bt, ref)
  msg = check(got)
  assert msg and 'wavefront' in msg[0] and 'lane offset' in msg[0], msg
  r = LM.tpw(bt.lpt) // 2 + 1
  assert not LM.check_bit_equal(bt, what, got, np.roll(got, r, 0), r)      # (the rotated run is wrong the same way)


def test_planted_unw_obs_error(small):
  """a 1e-4 relative error in one trajectory's unw_obs against unweighted_errors_batch"""
  bt = small[0]
  ok = LM.ok_rows(bt) & ~LM.near_decision(bt, bt.th)
  ref = LM.unweighted(bt, bt.th)[2]
  assert (ref[ok] > 0).sum() > bt.B // 2
  got = PC.rnd(ref, 'f32')
  assert not LM.check_close(bt, 'unw_obs', got[:, None], ref[:, None], LM.UNW_TOL['f32'], rows=ok)
  b = int(np.nonzero(ok & (ref > 0))[0][3])
  got[b] = ref[b] * (1 + 1e-4)
  msg = LM.check_close(bt, 'unw_obs', got[:, None], ref[:, None], LM.UNW_TOL['f32'], rows=ok)
  assert msg and 'trajectory %d ' % b in msg[0], msg


def test_planted_scalar_qc_lane_error():
  """'scalar' mode: a 1e-3 error in one lane's block gradients g_qc -- caught by the lane-resolved directional check over g_qc"""
  bt = LM.make(2, 16, 4, 64, 'scalar_diag', waves=6, seed=5)
  idx = np.array([0, 1, 3, 5]) * LM.tpw(bt.lpt)
  s = _subbatch(bt, idx)
  g, gbar, gext = _grads(bt, idx)
  grads = {k: g[k].reshape(LM.oracle_qc(s).shape if k == 'qc' else getattr(s, k).shape) for k in ('th', 'start', 'goal', 'qc', 'ow', 'eps')}
  v = LM.lane_direction_qc(s, grads['qc'])
  err, excl = LM.directional(s, grads, gbar, gext, v, nthreads=NTHREADS, h=LM.FD_H_QC)
  assert not excl.any() and err.max() < LM.FD_LANE_TOL, err
  lane = LM.probe_lane(s, 2)
  grads['qc'] = grads['qc'].copy(); grads['qc'][2, lane * s.c:(lane + 1) * s.c] *= 1 + 1e-3
  err2, _ = LM.directional(s, grads, gbar, gext, v, nthreads=NTHREADS, h=LM.FD_H_QC)
  assert err2[2] > 5 * LM.FD_LANE_TOL and (np.delete(err2, 2) < LM.FD_LANE_TOL).all(), err2


# ---- the GPU test body on the wavefront emulator ------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [(2, 16, 4, 64, 'perstate', True),       # per-state Kronecker, velocity limits, step-errors + tiled twins
                                 (3, 32, 4, 125, 'static', False),       # Woodbury ragged, traced loop + chain backward, step-errors + tiled twins
                                 (2, 64, 1, 61, 'qfull', False),         # general (q_full), one trajectory per wavefront
                                 (3, 16, 2, 32, 'static_full', False),   # general static, traced loop
                                 (2, 16, 4, 64, 'scalar_raw', False),    # DGP_QC_SCALAR through the raw output vector, step-errors + tiled twins
                                 (3, 16, 4, 64, 'static_diag', False),   # block elimination at C = 4 (variant 1), traced loop + chain backward
                                 (2, 32, 4, 125, 'perstate', True, LM.ODD_GRID)],      # per-sample grids of an odd size: the tiled twins on padded tiles
                         ids=lambda c: 'dof%d_%d_%d_n%d_%s' % c[:5] + ('_grids' if len(c) > 6 else ''))
def test_emulator_pipeline(cfg, monkeypatch):
  dof, lpt, c, n, cov, vel = cfg[:6]
  monkeypatch.setenv('DGP_FORCE_SHAPE', '%d,%d' % (lpt, c))
  bt = LM.make(dof, lpt, c, n, cov, vel=vel, waves=3 if lpt < 64 else 5, seed=11, grid=cfg[6] if len(cfg) > 6 else None)
  rep = {}
  bad = LM.run_config(harness.Backend('emul'), bt, nthreads=NTHREADS, report=rep)
  assert not bad, '\n'.join(bad[:40])
  assert rep['fd_worst'] < LM.FD_TOL and rep.get('b_excluded', 0) <= 1, rep
  if LM.expected_variant(lpt, c, n, cov, vel) is not None: assert rep['variant'] == (LM.expected_variant(lpt, c, n, cov, vel), c), rep
