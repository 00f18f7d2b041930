"""The per-trajectory SPD flag `info` against an inertia reference (host only): shared by tests/test_hip_spd_flag.py (GPU) and
tests/test_lane_emulator.py (the wavefront emulator).

`info[b] = 1` is the only failure signal of the solver: the reference raises from torch.cholesky where the kernels OR a ballot into a lane
mask (SpdCheck, gn_lane.h) that is cut into trajectory groups at the end of the kernel.  By Sylvester's law of inertia a symmetric matrix
that is not positive definite shows a non-positive pivot under ANY symmetric elimination order, so the verdict is a property of
LAM = A^T K A + reg I, not of PCR against Cholesky, and a reference is easy to state:

  * the extended-precision C oracle (oracle/gn_blocktri.c, the long-double build): its info, at every n;
  * for n d <= 256 the dense numpy oracle: eigvalsh(normal_equations(construct_linear_system_batch(...))).min() <= 0.

A trajectory is DECIDED when the long-double oracle returns the same verdict at reg - delta and reg + delta, delta = DELTA_REL |max diag(LAM)|
(shifting reg shifts every eigenvalue by exactly that much, so a decided trajectory has |lambda_min| > delta; elimination rounding is about
N u |LAM| <= 1536 x 1.1e-16 = 2e-13, 600 times below).  Only decided trajectories are compared; at most MAX_EXCLUDED of the trajectories of a
(configuration, rung) may be undecided / excluded, and every configuration has a rung on which one wavefront holds both a decided-clean and a
decided-flagged trajectory (check_conditions).

Inputs: the lane-mixed batches of tests/lane_mix.py at WAVES = 3 wavefronts (B = 14, 7 or 3, the last wavefront ragged), without NaN.
  lever A -- every covariance mode: the reg ladder rungs(cfg), +0.1 (the clean control) and negative rungs;
  lever B -- the modes with per-call covariance tensors (LEVER_B_COVS): one GP block of chosen trajectories times -50 at reg = +0.1
             (lever_b_picks: factors 0, (n-1)//2, n-2 and the one at the last non-padding lane; wavefront slots 0, last, middle and the
             ragged wavefront).
run_ladder / run_lever_b return lists of failure strings naming the configuration, the trajectory, its wavefront and its lane offset."""
import copy
import os
import numpy as np
import parity_cases as PC
import lane_mix as LM
from oracle import gpmp2_oracle as O
from oracle import blocktri as BT

WAVES = 3
DELTA_REL = 1e-10          # decided: the same verdict at reg -+ DELTA_REL |max diag(LAM)|
SOLVED_REL = 5e-6          # (c): dtheta is held to the oracle where LAM stays positive definite with reg lowered by SOLVED_REL |max diag(LAM)| (cond <= 2e5, PC.TOL's)
MAX_EXCLUDED = 0.10
K_LOOP = 3
BAND = 1e-6                # lane_mix.stopping's band around tol_delta
LADDER = (0.1, -0.01, -0.1, -1.0, -1.0e3, -1.0e7)
# rungs added where LADDER alone puts no decided-clean and decided-flagged trajectory into one wavefront (found on the CPU with the long-double oracle:
# find_mixed_rungs): keyed by (dof, lpt, c, n, cov), the per-sample-grid configuration by (..., ODD_GRID)
EXTRA_RUNGS = {(2, 16, 1, 16, 'static'): (-0.2,), (2, 16, 1, 16, 'static_diag'): (-0.2,), (2, 32, 1, 32, 'qfull'): (-0.02,), (2, 32, 2, 61, 'qfull'): (-0.002,),
               (2, 32, 4, 128, 'static_full'): (-2.0,), (2, 32, 4, 128, 'qfull'): (-0.001,), (3, 32, 4, 128, 'qfull'): (-0.001,),
               (2, 32, 4, 125, 'perstate', LM.ODD_GRID): (-2.0,)}
# a rung replaced: n = 1024, per-state blocks -- max diag(LAM) = 3.6e7, so delta = 3.6e-3 is a third of the rung -0.01, and the second iterate of one of the three
# trajectories is undecided there (the cap allows none of three); at -0.03 every iterate of every trajectory is decided and one trajectory is flagged by the loop only
REPLACED_RUNGS = {(2, 64, 16, 1024, 'perstate'): {-0.01: -0.03}}
LEVER_B_COVS = ('perstate', 'qfull', 'scalar', 'scalar_diag')      # (not 'scalar_raw': its values are squared)
LEVER_B_FACTOR = -50.0


def long_configs(dof):
  """the loop kernels of gn_long.h (n > 256): test_hip_full_batch_long_trajectories' lengths and modes"""
  return [(64, -(-n // 64), n, cov, dof == 2 and cov == 'static') for n, cov in ((257, 'static'), (257, 'qfull'), (1024 if dof == 2 else 640, 'perstate'))]


def all_configs(dof):
  """[(cfg = (lpt, c, n, cov, vel), grid, seed)]: lane_mix.configs, odd_config and the long cases, seeded as tests/test_hip_full_batch.py seeds them"""
  out = [(cf, None, 1000 * dof + 10 * cf[0] + cf[1]) for cf in LM.configs(dof)]
  cf = LM.odd_config(dof)
  out.append((cf, LM.ODD_GRID, 1000 * dof + 10 * cf[0] + cf[1] + 5))
  out += [(cf, None, 77 + cf[2]) for cf in long_configs(dof)]
  return out


def batch(dof, cfg, grid=None, seed=0):
  lpt, c, n, cov, vel = cfg
  bt = LM.make(dof, lpt, c, n, cov, vel=vel, waves=WAVES, seed=seed, nan=False, grid=grid)
  bt.long = n > 256
  bt.key = (dof, lpt, c, n, cov)
  bt.ref_key = bt.key + (grid, seed)      # (the per-sample-grid configuration shares its key with one of lane_mix.configs)
  return bt


def rungs(bt):
  key = bt.key if bt.ref_key[5] is None else bt.key + (bt.ref_key[5],)
  rep = REPLACED_RUNGS.get(key, {})
  return tuple(rep.get(r, r) for r in LADDER) + tuple(EXTRA_RUNGS.get(key, ()))


def _params(p, reg):
  q = copy.copy(p); q.reg = float(reg)
  return q


def with_reg(bt, reg):
  out = LM.Batch(); out.__dict__.update(bt.__dict__)
  out.p = _params(bt.p, reg)
  return out


def sub(bt, idx):
  """the trajectories idx as a batch of their own"""
  idx = np.asarray(idx)
  s = LM.Batch(); s.__dict__.update(bt.__dict__)
  for k in ('th', 'th_clean', 'start', 'goal', 'qc', 'ow', 'eps', 'qc_dense', 'raw_out'):
    a = getattr(bt, k); setattr(s, k, None if a is None else a[idx])
  if bt.sdf.shape[0] == bt.B and bt.B > 1: s.sdf = bt.sdf[idx]
  s.B = len(idx); s.nan_rows = np.zeros(0, np.int64)
  return s


# ---- references -------------------------------------------------------------------------------------------------------------------------------
def _covs_dense(bt):
  """(Q_inv (B,n-1,d,d), obs_w (B,n,1,1), eps (B,n,1,1)) as construct_linear_system_batch takes them"""
  sq, so, se = bt.p.static_covs(bt.B)
  qc = LM.oracle_qc(bt)
  Q = (sq if qc is None else qc)
  Q = Q if bt.q_full else O.calc_Q_inv_batch(Q, bt.p.dt)
  return Q, (so if bt.ow is None else bt.ow.reshape(so.shape)), (se if bt.eps is None else bt.eps.reshape(se.shape))


def _sdf_full(bt):
  return np.broadcast_to(bt.sdf, (bt.B,) + bt.sdf.shape[1:])


def diag_lam(bt, th, reg):
  """diag(LAM) (B, n d) from the diagonal blocks alone (any n): the factors' Jacobians of oracle.gpmp2_oracle, assembled as construct_linear_system_batch
  assembles them -- held to the dense LAM by tests/test_lane_emulator.py"""
  p = bt.p
  B, n, d = th.shape
  assert not (p.non_holonomic and p.use_vel_limits)
  Q, ow, eps = _covs_dense(bt)
  phi = O.calc_phi(p.dof, p.dt)
  dg = np.zeros((B, n, d))
  dg[:, 0] += 1.0 / p.K_s ** 2.0; dg[:, n - 1] += 1.0 / p.K_g ** 2.0
  dg[:, 1:] += np.einsum('bkii->bki', Q)                         # H2 = -I
  dg[:, :-1] += np.einsum('ia,bkij,ja->bka', phi, Q, phi)        # H1 = Phi
  _, H = O.obstacle_error(th, _sdf_full(bt), eps, p)
  dg += ow.reshape(B, n, 1) * H[:, :, 0] ** 2
  if p.non_holonomic: dg += (1.0 / p.K_d ** 2.0) * O.nonholonomic_error(th)[1][:, :, 0] ** 2
  if p.use_vel_limits: dg += (1.0 / p.K_v ** 2.0) * (O.vel_limit_error(th, p)[1] ** 2).sum(2)
  return dg.reshape(B, n * d) + reg


def dense_lam(bt, th, reg):
  """LAM (B, n d, n d) of the dense numpy oracle"""
  Q, ow, eps = _covs_dense(bt)
  A, b, K = O.construct_linear_system_batch(th, bt.start, bt.goal, _sdf_full(bt), Q, ow, eps, bt.p)
  return O.normal_equations(A, b, K, reg)[0]


def oracle_step(bt, th, reg, nthreads=1):
  """the long-double C oracle at `reg` -> dtheta (NaN where flagged), info"""
  d, _, _, info = BT.gn_step(_params(bt.p, reg), th, bt.start, bt.goal, bt.sdf, nthreads=nthreads, extended=True, **LM.okw(bt))
  return d, info


def verdict_at(bt, th, regs):
  """the long-double oracle's info with one reg PER TRAJECTORY"""
  out = np.zeros(bt.B, np.int32)
  for b in range(bt.B):
    s = sub(bt, [b])
    out[b] = BT.gn_step(_params(bt.p, regs[b]), th[b:b + 1], s.start, s.goal, s.sdf, extended=True, **LM.okw(s))[3][0]
  return out


class Ref(object):
  pass


def reference(bt, reg, th=None, nthreads=1):
  """-> Ref: verdict (B,) the long-double oracle's info at reg, decided (B,) bool, solved (B,) bool (positive definite at reg - SOLVED_REL |max diag|),
  dth the oracle's step (NaN where flagged), scale (B,) = |max diag(LAM)|"""
  th = bt.th if th is None else th
  r = Ref()
  r.scale = np.abs(diag_lam(bt, th, reg).max(1))
  delta = DELTA_REL * r.scale
  lo, hi = verdict_at(bt, th, reg - delta), verdict_at(bt, th, reg + delta)
  r.dth, r.verdict = oracle_step(bt, th, reg, nthreads)
  r.decided = lo == hi
  assert (r.verdict[r.decided] == lo[r.decided]).all() and (lo >= hi).all(), 'the verdict is not monotone in reg'
  r.solved = verdict_at(bt, th, reg - SOLVED_REL * r.scale) == 0
  return r


def median_tol(dth):
  """lane_mix.median_tol over the trajectories with a finite step (the flagged ones of a negative rung have none); a single one: half its norm
  (lane_mix.median_tol would return the norm itself, and the stopping rule would hang on its rounding)"""
  fin = np.isfinite(dth.reshape(dth.shape[0], -1)).all(1)
  if not fin.any(): return 1.0
  return LM.median_tol(dth[fin]) * (0.5 if fin.sum() == 1 else 1.0)


def chain_reference(bt, reg, tol, K=K_LOOP, io_round=False, nthreads=1):
  """The loops' info: the OR of the reference verdicts at the iterates trajectory b itself steps from (k < iters[b]), the long-double oracle chained under
  the loop's stopping rule.  -> flag (B,) int, excluded (B,) bool: the chain met an undecided iterate, or a step norm within BAND of tol, before any flag
  (a trajectory flagged once stays flagged whatever follows)."""
  cur = bt.th.copy(); on = np.ones(bt.B, bool); flag = np.zeros(bt.B, np.int32); excl = np.zeros(bt.B, bool)
  for k in range(K):
    if not on.any(): break
    r = reference(bt, reg, cur, nthreads)
    excl |= on & ~r.decided
    flag[on & r.decided & (r.verdict == 1)] = 1
    step = on & r.decided & (r.verdict == 0)
    nrm = np.sqrt((np.nan_to_num(r.dth).reshape(bt.B, -1) ** 2).sum(1))
    excl |= step & (np.abs(nrm - tol) <= BAND * tol)
    cur[step] += r.dth[step]
    if io_round: cur = PC.rnd(cur, 'f32')
    on = step & ~(nrm < tol) & ~excl
  return flag, excl


def mixed_waves(bt, r):
  """wavefronts that hold a decided-clean AND a decided-flagged trajectory"""
  T = LM.tpw(bt.lpt)
  wave = np.arange(bt.B) // T
  W = wave.max() + 1
  c = np.bincount(wave[r.decided & (r.verdict == 0)], minlength=W) > 0
  f = np.bincount(wave[r.decided & (r.verdict == 1)], minlength=W) > 0
  return np.nonzero(c & f)[0]


_REFS = {}


def references(bt, nthreads=1):
  """{rung: (Ref at th_init, tol_delta, chain flag, chain excluded)}: computed once per batch, shared by both I/O types (lane_mix's numbers are fp32-exact)
  and by every entry point; never modified"""
  key = (bt.ref_key, bt.B)
  if key not in _REFS:
    out = {}
    for reg in rungs(bt):
      r = reference(bt, reg, nthreads=nthreads)
      tol = median_tol(r.dth)
      chains = {}
      if not LM.is_scalar(bt.cov):
        for io_round in ((False, True) if bt.long else (False,)): chains[io_round] = chain_reference(bt, reg, tol, io_round=io_round, nthreads=nthreads)
      out[reg] = (r, tol, chains)
    _REFS[key] = out
  return _REFS[key]


def check_conditions(bt, refs, report=None):
  """the two conditions on the inputs, from the oracle alone: <= MAX_EXCLUDED undecided / excluded per rung; a mixed wavefront on some rung (T >= 2)"""
  bad = []
  rep = {} if report is None else report
  any_mixed = False
  for reg, (r, tol, chains) in refs.items():
    und = (~r.decided).sum()
    worst = max([und] + [int(ex.sum()) for _, ex in chains.values()])
    rep[reg] = dict(clean=int((r.decided & (r.verdict == 0)).sum()), flagged=int((r.decided & (r.verdict == 1)).sum()), undecided=int(und), excluded=int(worst),
                    mixed_waves=len(mixed_waves(bt, r)))
    if worst > MAX_EXCLUDED * bt.B: bad.append('%s reg %g: %d of %d trajectories undecided / excluded' % (bt.tag, reg, worst, bt.B))
    any_mixed |= len(mixed_waves(bt, r)) > 0
  if LM.tpw(bt.lpt) >= 2 and not any_mixed: bad.append('%s: no rung with a decided-clean and a decided-flagged trajectory in one wavefront' % bt.tag)
  return bad


def find_mixed_rungs(bt, candidates=None):
  """the rungs among `candidates` (default: a log grid of negative reg) that give a mixed wavefront -- the search behind EXTRA_RUNGS"""
  cand = [-m * 10.0 ** e for e in range(-4, 5) for m in (1.0, 2.0, 5.0)] if candidates is None else candidates
  return [reg for reg in cand if len(mixed_waves(bt, reference(bt, reg)))]


# ---- checks against a backend -------------------------------------------------------------------------------------------------------------------
def _flag_fails(bt, what, info, want, rows):
  """(a): info == the reference verdict on `rows`, in both directions"""
  info = np.asarray(info)
  return ['%s %s: info %d, reference %d: %s' % (bt.tag, what, info[b], want[b], LM._where(bt, b)) for b in np.nonzero(rows & (info != want))[0]]


def _env(name, value):
  class _E(object):
    def __enter__(s):
      s.old = os.environ.get(name)
      if value is None: os.environ.pop(name, None)
      else: os.environ[name] = value
    def __exit__(s, *a):
      if s.old is None: os.environ.pop(name, None)
      else: os.environ[name] = s.old
  return _E()


def families(bt):
  """the entry points next to dgp_gn_step that exist for this batch (lane_mix.run_config's rule)"""
  fam = []
  if not LM.is_scalar(bt.cov): fam.append('solve')
  if bt.long: return fam
  if bt.cov in ('static', 'static_diag', 'static_full'): fam.append('traced')
  if bt.c == 4 and bt.lpt <= 32: fam += ['step_errors', 'tiled']
  return fam


def _tiled(be):
  import harness
  t = harness.Backend(be.kind); t.sdf_tiled = True
  return t


def _run_all(be, bt, io, tol, fam):
  """every entry point on one batch -> {name: outputs}; 'step' (dtheta, err, err_ext, info), 'step_errors' (+ unw_*), 'tiled', 'solve' / 'traced' (info,)"""
  kw = LM.kkw(bt, io)
  a = (bt.p, bt.th, bt.start, bt.goal, bt.sdf)
  o = {'step': be.step(*a, **kw)}
  if 'step_errors' in fam: o['step_errors'] = be.step_errors(*a, **kw)
  if 'tiled' in fam: o['tiled'] = _tiled(be).step(*a, **kw)
  if 'solve' in fam: o['solve'] = (be.solve(*a, K_LOOP, tol, **kw)[5],)
  if 'traced' in fam: o['traced'] = (be.solve_traced(*a, K_LOOP, tol, io=io)[3],)
  return o


def _info(name, out):
  return out[0] if name in ('solve', 'traced') else out[3]


def trimmed_rungs(bt, refs):
  """the emulator's selection: the clean control, the first rung that mixes clean and flagged trajectories (inside a wavefront where the shape has one),
  and -1e3 (every trajectory flagged)"""
  mixed = [reg for reg, (r, _, _) in refs.items() if len(mixed_waves(bt, r))] or [reg for reg, (r, _, _) in refs.items() if 0 < (r.decided & (r.verdict == 1)).sum() < bt.B]
  return (LADDER[0],) + tuple(mixed[:1]) + (-1.0e3,)


def run_ladder(be, bt, io, nthreads=1, report=None, variant=True, alone=True, rotation=True, only=None):
  """Lever A on one configuration, one I/O type: (a), (c), (d), (e) of tests/test_hip_spd_flag.py on every rung (`only`: on those rungs) -> list of failures"""
  from dgpmp2_amd import _capi
  import harness
  bad = []
  rep = {} if report is None else report
  refs = references(bt, nthreads)
  bad += check_conditions(bt, refs, rep)
  fam = families(bt)
  cfg = (bt.lpt, bt.c, bt.n, bt.cov, bt.p.use_vel_limits)
  want_v = LM.expected_variant(*cfg)
  passes = [None] + (['1'] if want_v in (3, 4) else [])      # Woodbury configurations a second time with DGP_NO_WOODBURY=1 (block elimination, variant 1)
  T = LM.tpw(bt.lpt)
  rot = T // 2 + 1
  for nowb in passes:
    with _env('DGP_NO_WOODBURY', nowb):
      if variant and want_v is not None:
        got = _capi.Solver(harness.config_from_oracle(bt.p, 'f64'), api=be.api).step_kernel_variant(bt.B)
        if got != (want_v if nowb is None else 1): bad.append('%s: static kernel variant %d, expected %d' % (bt.tag, got, want_v if nowb is None else 1))
      for reg, (r, tol, chains) in refs.items():
        if only is not None and reg not in only: continue
        t = '[%s]%s reg %g ' % (io, '' if nowb is None else ' [no Woodbury]', reg)
        b_ = with_reg(bt, reg)
        o = _run_all(be, b_, io, tol, fam)
        flag, excl = chains.get(bt.long and io == 'f32', (None, None))
        for name, out in o.items():
          info = _info(name, out)
          if name in ('solve', 'traced'):
            bad += _flag_fails(bt, t + name, info, flag, ~excl)                                                  # (e) the chained reference
            bad += ['%s %s%s: flagged by the step at th_init, not by the loop: %s' % (bt.tag, t, name, LM._where(bt, b))
                    for b in np.nonzero((_info('step', o['step']) != 0) & (info == 0))[0]]
          else:
            bad += _flag_fails(bt, t + name, info, r.verdict, r.decided)                                         # (a)
            rows = r.decided & (r.verdict == 0) & r.solved                                                       # (c) clean trajectories are still solved
            if reg < 0 and rows.any(): bad += LM.check_close(bt, t + name + ' dtheta', out[0], np.nan_to_num(r.dth), (10 if bt.n > 512 else 1) * PC.TOL[io], rows=rows)
        rep.setdefault('solved_checked', {})[reg] = int((r.decided & (r.verdict == 0) & r.solved).sum())
        if rotation:                                                                                             # (d) purity: rotated by TPW // 2 + 1 trajectories
          ro = _run_all(be, LM.rotate(b_, rot), io, tol, [f for f in fam if f in ('solve', 'traced')])
          for name, out in ro.items(): bad += LM.check_bit_equal(bt, t + name + ' info', _info(name, o[name]), _info(name, out), rot)
        if alone and nowb is None:                                                                               # (d) a decided trajectory alone (B = 1)
          picks = [np.nonzero(r.decided & (r.verdict == v))[0] for v in (0, 1)]
          mw = mixed_waves(bt, r)
          if len(mw): picks = [pk[pk // T == mw[0]] for pk in picks]
          for pk in picks:
            if not len(pk): continue
            b = int(pk[-1])
            s = with_reg(sub(bt, [b]), reg)
            one = _run_all(be, s, io, tol, [f for f in fam if f == 'solve'])
            for name, out in one.items():
              if _info(name, out)[0] != _info(name, o[name])[b]:
                bad.append('%s %s%s: info %d alone (B = 1), %d inside the batch: %s' % (bt.tag, t, name, _info(name, out)[0], _info(name, o[name])[b], LM._where(bt, b)))
  return bad


# ---- lever B -----------------------------------------------------------------------------------------------------------------------------------
def lever_b_picks(bt):
  """[(trajectory, GP factor)]: factors 0, (n-1)//2, n-2 and the one at the first state of the last non-padding lane; trajectories at wavefront slot 0, the last
  slot, a middle slot and in the ragged last wavefront (T = 1: two of the three trajectories, two placements -> a list of placements)"""
  n, c, T, B = bt.n, bt.c, LM.tpw(bt.lpt), bt.B
  jl = (n - 1) // c
  k_last = jl * c if jl * c < n - 2 else max(0, jl * c - 1)
  ks = [0, (n - 1) // 2, n - 2, k_last]
  if T == 1: return [[(0, ks[0]), (2, ks[2])], [(1, ks[1]), (2, ks[3])]]
  return [[(0, ks[0]), (T + T - 1, ks[1]), (2 * T + T // 2, ks[2]), (B - 1, ks[3])]]


def negate_blocks(bt, picks):
  """the batch with qc[b, k] -> -50 qc[b, k] for (b, k) in picks (rounded to fp32 like every number of the batch)"""
  out = LM.Batch(); out.__dict__.update(bt.__dict__)
  out.qc = bt.qc.copy()
  for b, k in picks: out.qc[b, k] = PC.rnd(LEVER_B_FACTOR * bt.qc[b, k], 'f32')
  if LM.is_scalar(bt.cov): out.qc_dense = out.qc[:, :, None, None] * bt.p.Q_c_inv
  return out


def run_lever_b(be, bt, io, nthreads=1, report=None):
  """Lever B on one configuration: (a) on the batch with the negated blocks, (b) isolation of every trajectory that was not made bad -> failures"""
  bad = []
  rep = {} if report is None else report
  fam = families(bt)
  reg = bt.p.reg
  tol = references(bt, nthreads)[reg][1]
  clean = _run_all(be, bt, io, tol, fam)
  for pi, picks in enumerate(lever_b_picks(bt)):
    bb = negate_blocks(bt, picks)
    chosen = np.zeros(bt.B, bool); chosen[[b for b, _ in picks]] = True
    ck = (bt.ref_key, bt.B, 'B', pi)      # (the references of the negated batch: once for both I/O types, like references())
    if ck not in _REFS:
      _REFS[ck] = (reference(bb, reg, nthreads=nthreads),
                   {x: chain_reference(bb, reg, tol, io_round=x, nthreads=nthreads) for x in ((False, True) if bt.long else (False,))} if 'solve' in fam else {})
    r, chains = _REFS[ck]
    t = '[%s] lever B %s ' % (io, picks)
    for b, k in picks:
      if not (r.decided[b] and r.verdict[b] == 1): bad.append('%s %s: the oracle does not flag %s (factor %d)' % (bt.tag, t, LM._where(bt, b), k))
    if bt.n * 2 * bt.dof <= 256:      # the dense oracle confirms lambda_min < -delta
      lmin = np.linalg.eigvalsh(dense_lam(bb, bb.th, reg)).min(1)
      for b, k in picks:
        if not lmin[b] < -DELTA_REL * r.scale[b]: bad.append('%s %s: dense lambda_min %.3g of %s' % (bt.tag, t, lmin[b], LM._where(bt, b)))
    rep['lever_b_%d' % pi] = dict(flagged=int((r.decided & (r.verdict == 1)).sum()), clean=int((r.decided & (r.verdict == 0)).sum()), undecided=int((~r.decided).sum()))
    if (~r.decided).sum() > MAX_EXCLUDED * bt.B: bad.append('%s %s: %d undecided trajectories' % (bt.tag, t, (~r.decided).sum()))
    o = _run_all(be, bb, io, tol, fam)
    chain = chains.get(bt.long and io == 'f32')
    for name, out in o.items():
      info = _info(name, out)
      if name in ('solve', 'traced'): bad += _flag_fails(bt, t + name, info, chain[0], ~chain[1])
      else: bad += _flag_fails(bt, t + name, info, r.verdict, r.decided)
      names = ('info',) if name in ('solve', 'traced') else ('dtheta', 'err', 'err_ext', 'info', 'unw_sg', 'unw_gp', 'unw_obs')
      for nm, x, y in zip(names, out, clean[name]):                                       # (b) isolation, bit for bit
        for b in np.nonzero(~chosen)[0]:
          if not np.array_equal(np.asarray(x[b]), np.asarray(y[b]), equal_nan=np.asarray(x).dtype.kind == 'f'):
            bad.append('%s %s%s %s: a negated block of %s reached %s' % (bt.tag, t, name, nm, [p_ for p_ in picks if p_[0] // LM.tpw(bt.lpt) == b // LM.tpw(bt.lpt)], LM._where(bt, b)))
  return bad
