"""Call forms: the same mathematics reached through another launch.  Two things change which code a launch runs without changing its results -- WHICH
OPTIONAL POINTERS ARE NULL (wave-uniform branches around real work: the adjoint solve, the staged block store of g_th, every optional output) and WHETHER
EACH BUFFER IS 16-BYTE ALIGNED (dgp_host.h sets vec_io / vec_mu / vec_qc per call from the pointers: vector or scalar row access, block_rows).  PlanLayer
uses both on every training step.  Shared by tests/test_hip_call_forms.py (GPU: every kernel instantiation) and tests/test_lane_emulator.py (CPU emulator).

For one configuration (robot, I/O type, forced launch shape, length, covariance family, grid ownership / layout) and each entry point of a group:
  (a) the CANONICAL call -- everything present, aligned, guard bands on -- is pinned: forward outputs to the C oracle (oracle/gn_blocktri.c, chained for
      the loop) at PC.TOL / PC.TOL_ERR / 1e-7 | 1e-5; in the (16,4) shapes the backward to torch autograd over the dense restatement
      (oracle/autograd_torch.py) at that test's 1e-6 | 2e-3 F32_GRAD_SCALE, the chain and step-errors backward to the pinned single launches they fuse;
  (b) NULL forms -- each optional argument absent alone, each present alone, all absent, and PlanLayer's two patterns (covariance gradients only; g_th only):
      every output that is present must be np.array_equal to the canonical one.  A NULL cotangent is compared with an explicit zero cotangent the same way;
  (c) alignment forms -- every buffer one element past a 16-byte boundary, inputs only, outputs only, and one of them together with "all absent".
Every call runs with harness guard bands (no store outside an output, no store into an input).

The grid gradient: per-sample grids run DGP_GSDF_SPARSE, tap values AND indices bit-equal.  Shared grids run DGP_GSDF_DENSE_F64 with 1 or 16 partial copies,
summed over the copies and held at 1e-12 of max |g_sdf|: float64 atomics land in an order that changes from run to run (the bound of
parity_cases.case_unaligned_buffers).  Dense grids of fp32 I/O are NOT compared: their fp32 atomics move the sum by more than rounding (lane_mix.py) -- that is
the only quantity a call form may move, and it is kept out (long trajectories with fp32 I/O have no other delivery: their grid gradient is only guarded).
"""
import contextlib
import os
import numpy as np
import parity_cases as PC
from oracle import gpmp2_oracle as O, blocktri as BT

F32_GRAD_SCALE = float(os.environ.get('DGP_F32_GRAD_SCALE', 1.0))
SHAPES = [(l, c) for l in (16, 32, 64) for c in (1, 2, 4)]
COVS = ['static', 'static_diag', 'static_full', 'perstate', 'qfull', 'scalar']
GROUPS = ('forward', 'backward', 'loop', 'errs')
K = 3                                   # loop iterations
HW = (24, 40)
ALIGN = (True, 'inputs', 'outputs')     # harness.Backend.misalign
ORDER_TOL = 1e-12                       # float64 atomics of a shared grid's gradient (relative to max |g_sdf|)


class Cfg(object):
  """grid: 'per' (one grid per trajectory, sparse gradient), 'shared1' / 'shared16' (one grid, float64 gradient in 1 / 16 partial copies), 'dense' (long trajectories)"""

  def __init__(self, dof, io, shape, n, cov, grid='shared1', tiled=False, B=None):
    self.dof, self.io, self.shape, self.n, self.cov, self.grid, self.tiled = dof, io, shape, n, cov, grid, tiled
    self.B = B if B is not None else (64 // shape[0] + 1 if shape else 5)      # one full wavefront (block_rows, the vector row I/O live) and a partial one

  def tag(self):
    return 'dof %d %s shape %s n %d cov %s grid %s%s B %d' % (self.dof, self.io, self.shape, self.n, self.cov, self.grid, ' tiled' if self.tiled else '', self.B)


def lengths(lpt, c): return (lpt * c, max(4, lpt * c - 3))


@contextlib.contextmanager
def forced_shape(shape):
  old = os.environ.get('DGP_FORCE_SHAPE')
  if shape is None: os.environ.pop('DGP_FORCE_SHAPE', None)
  else: os.environ['DGP_FORCE_SHAPE'] = '%d,%d' % shape
  try: yield
  finally:
    if old is None: os.environ.pop('DGP_FORCE_SHAPE', None)
    else: os.environ['DGP_FORCE_SHAPE'] = old


def make_inputs(rs, c):
  """the inputs of tests/test_hip_every_kernel.py (24 x 40 grid, three circles, a noisy straight line), plus the scaled family and per-sample grids"""
  dof, n, B, io = c.dof, c.n, c.B, c.io
  d = 2 * dof
  kw = {}
  if dof == 3: kw.update(non_holonomic=True, K_d=0.1)
  if c.cov == 'static_full':
    A = rs.randn(dof, dof) * 0.3
    kw['Q_c_inv'] = np.eye(dof) + A @ A.T
  if c.cov == 'static_diag': kw['Q_c_inv'] = np.diag(1.0 + 0.5 * np.arange(dof))
  p = O.OracleParams(dof=dof, total_time_step=n - 1, reg=0.1, epsilon_dist=0.3, **kw)
  H, W = HW
  # A shared grid's gradient is summed by atomics in an order that changes from run to run.  A state outside the grid's 24 rows (y < -0.75 at the default limits: res = 10 / 40)
  # has clamped, coinciding taps whose weights cancel -- pairs of +-5e5 on ONE cell that sum to zero exactly only in a fixed order, 5e-11 of noise otherwise, on a gradient of
  # O(10).  So the shared-grid configurations keep their trajectories and obstacles inside the rows (the sum is then held at ORDER_TOL); the per-sample ones, which are compared
  # bit for bit, keep the clamped states.
  inside = c.grid != 'per'
  ylo, yhi = (-0.25, 4.25) if inside else (-4.0, 4.0)
  yy, xx = np.meshgrid((5.0 - 0.25 * np.arange(H)) if inside else np.linspace(5, -5, H), np.linspace(-5, 5, W), indexing='ij')
  cs = rs.uniform(-3, 3, (3, 2)); rr = rs.uniform(0.4, 1.2, 3)
  if inside: cs[:, 1] = rs.uniform(0.5, 3.5, 3)
  sdf = np.min(np.sqrt((xx[None] - cs[:, 0, None, None]) ** 2 + (yy[None] - cs[:, 1, None, None]) ** 2) - rr[:, None, None], axis=0)[None, None]
  if c.grid == 'per': sdf = np.concatenate([sdf + 0.05 * rs.randn() for _ in range(B)], 0)
  start = np.zeros((B, 1, d)); goal = np.zeros((B, 1, d))
  start[:, 0, :2] = rs.uniform(-4, 4, (B, 2)); goal[:, 0, :2] = rs.uniform(-4, 4, (B, 2))
  start[:, 0, 1] = rs.uniform(ylo, yhi, B); goal[:, 0, 1] = rs.uniform(ylo, yhi, B)
  if dof == 3: goal[:, 0, 2] = rs.uniform(-np.pi, np.pi, B)
  th = O.straight_line_trajb(start[:, :, :dof], goal[:, :, :dof], 10.0, n - 1, dof) + rs.randn(B, n, d) * 0.03
  qc = ow = eps = None; q_full = False
  if c.cov in ('perstate', 'qfull', 'scalar'):
    ow = rs.uniform(50, 2e4, (B, n)); eps = rs.uniform(0.1, 0.6, (B, n))
    if c.cov == 'perstate':
      A = rs.randn(B, n - 1, dof, dof) * 0.2; qc = np.eye(dof) + A @ np.swapaxes(A, -1, -2)
    elif c.cov == 'qfull':
      A = rs.randn(B, n - 1, d, d) * 0.2; qc = (np.eye(d) + A @ np.swapaxes(A, -1, -2)) * 1.5; q_full = True
    else:
      qc = rs.uniform(0.3, 3.0, (B, n - 1)) ** 2
  r = lambda a: None if a is None else PC.rnd(a, io)
  return p, r(th), r(start), r(goal), r(sdf), r(qc), r(ow), r(eps), q_full


def null_forms(opt, extra=(), valid=None):
  """each optional argument absent alone, each present alone, all absent, then `extra` -- as tuples of absent names, duplicates dropped.
  valid(form) -> the form made legal (e.g. th_hist needs iters)"""
  opt = tuple(opt)
  forms = [(o,) for o in opt] + [tuple(x for x in opt if x != o) for o in opt] + [opt] + [tuple(e) for e in extra]
  seen, out = set(), []
  for f in forms:
    if valid is not None: f = valid(f)
    key = frozenset(f)
    if f and key not in seen: seen.add(key); out.append(tuple(f))
  return out


class Run(object):
  """one configuration: inputs, the failure list, the comparisons"""

  def __init__(self, be, c, fails, oracle=True):
    self.be, self.c, self.fails, self.oracle = be, c, fails, oracle
    self.rs = np.random.RandomState(1000 * c.dof + 100 * (c.io == 'f32') + 7 * c.n + (c.shape[0] + c.shape[1] if c.shape else 3) + 13 * COVS.index(c.cov) + len(c.grid))
    self.p, self.th, self.start, self.goal, self.sdf, self.qc, self.ow, self.eps, self.q_full = make_inputs(self.rs, c)
    self.kw = dict(qc=self.qc, ow=self.ow, eps=self.eps, q_full=self.q_full, io=c.io)
    sh = (c.B, c.n, 1, 1)
    dense = None if self.qc is None else (self.qc[:, :, None, None] * np.eye(c.dof) if c.cov == 'scalar' else self.qc)
    self.okw = dict(qc=dense, ow=None if self.ow is None else self.ow.reshape(sh), eps=None if self.eps is None else self.eps.reshape(sh), q_full=self.q_full)
    self.a = (self.p, self.th, self.start, self.goal, self.sdf)
    self.gm = dict(sdf_grad='sparse') if c.grid == 'per' else (dict(sdf_grad='dense') if c.grid == 'dense' else dict(sdf_grad='f64', sdf_copies=16 if c.grid == 'shared16' else 1))
    self.pin16 = oracle and c.shape == (16, 4)      # where the backward is held to the dense autograd oracle
    self.k = 0
    self.compared = 0

  def bad(self, form, name, what): self.fails.append((self.c.tag(), form, name, what))

  def pin(self, form, name, a, ref, tol, scale=None, per_traj=False):
    """canonical result against an oracle"""
    if a is None or not np.all(np.isfinite(a)): return self.bad(form, name, 'missing / non-finite')
    ref = np.asarray(ref, dtype=np.float64).reshape(a.shape)
    e = PC.rel_err_per_traj(a, ref) if per_traj else float(np.abs(a - ref).max() / max(np.abs(ref).max(), 0.0 if scale is None else np.abs(scale).max(), 1e-300))
    if not e < tol: self.bad(form, name, 'oracle: %.3g (bound %.3g)' % (e, tol))

  def rowmajor(self, call):
    """call() on the row-major grid: what a grid-free launch (sdf = NULL) is held to -- without a grid there is no layout, so it runs the standard kernels at the
    standard shape choice (dgp_host.h choose_kernel: `tiled = p.sdf_layout != 0 && p.sdf != nullptr`), which for a tiled grid under a forced (64,4) is another shape
    than the twin's (tiled_shape_ok) and sums a trajectory's errors over other lanes"""
    old = self.be.sdf_tiled
    self.be.sdf_tiled = False
    try: return call()
    finally: self.be.sdf_tiled = old

  def grads(self, r):
    """a backward's dict, the sparse arrays as delivered next to the scattered grid"""
    r = dict(r)
    if r.get('sdf') is not None and self.c.grid == 'per': r['sdf_vals'], r['sdf_idx'] = self.be.last_sparse
    return r

  def compare(self, form, out, can):
    """every present output of a variant against the pinned canonical result: bit-equal (the float64 grids of a shared grid: ORDER_TOL)"""
    for name, ref in can.items():
      a = out.get(name)
      if a is None: continue
      self.compared += 1
      if ref is None: self.bad(form, name, 'present in the variant only'); continue
      if name == 'sdf' and self.c.grid != 'per':
        if self.c.grid == 'dense' and self.c.io == 'f32': continue      # fp32 atomics: not compared (module docstring)
        a, ref = a.sum(0, keepdims=True), ref.sum(0, keepdims=True)      # (the partial copies)
        e = float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if np.all(np.isfinite(a)) else np.inf
        if not e < ORDER_TOL: self.bad(form, name, '%.3g (bound %.3g)' % (e, ORDER_TOL))
      elif not (a.shape == ref.shape and np.array_equal(a, ref, equal_nan=True)):
        with np.errstate(invalid='ignore'):
          self.bad(form, name, 'not bit-equal: %d entries, %d NaN' % (int((a != ref).sum()), int(np.isnan(a).sum())) if a.shape == ref.shape else 'shape')

  def sweep(self, what, call, opt, can, extra=(), valid=None, ref=None):
    """(b) and (c) for one entry point; call(absent) -> dict of outputs.  ref(absent) -> the pinned result a form is held to where it is not `can` (a form that BY DESIGN
    launches another kernel)"""
    be = self.be
    ref = ref or (lambda ab: can)
    for ab in null_forms(opt, extra, valid): self.compare('%s NULL %s' % (what, ','.join(ab)), call(ab), ref(ab))
    try:
      for mis in ALIGN:
        be.misalign = mis
        self.compare('%s misaligned %s' % (what, mis), call(()), can)
      be.misalign = ALIGN[self.k % 3]; self.k += 1
      ab = tuple(opt) if valid is None else valid(tuple(opt))
      self.compare('%s misaligned %s + all NULL' % (what, be.misalign), call(ab), ref(ab))
    finally:
      be.misalign = False


STEP_NAMES = ('dtheta', 'err', 'err_ext', 'info')
EVAL_NAMES = ('err', 'err_ext', 'unw_sg', 'unw_gp', 'unw_obs')
SOLVE_NAMES = ('th_out', 'iters', 'err_hist', 'errext_hist', 'err_final', 'info')
ERRS_NAMES = ('dtheta', 'err', 'err_ext', 'info', 'unw_sg', 'unw_gp', 'unw_obs')


def _pin_step(R, what, can):
  io = R.c.io
  o = BT.gn_step(*R.a, **R.okw)
  R.pin(what, 'dtheta', can['dtheta'], o[0], PC.TOL[io], per_traj=True)
  R.pin(what, 'err', can['err'], o[1], PC.TOL_ERR[io]); R.pin(what, 'err_ext', can['err_ext'], o[2], PC.TOL_ERR[io])
  if can['info'] is None or can['info'].any(): R.bad(what, 'info', 'set')


def _pin_unw(R, what, can, th):
  B = R.c.B
  eps = np.full((B, R.c.n, 1, 1), R.p.epsilon_dist) if R.eps is None else R.eps.reshape(B, R.c.n, 1, 1)
  sg, gp, ob = O.unweighted_errors_batch(th, R.start, R.goal, np.broadcast_to(R.sdf, (B,) + R.sdf.shape[1:]), eps, R.p)
  # (the bound of test_hip_every_step_errors_kernel for these three: the start / goal error is a difference of nearly equal numbers)
  tol = 1e-10 if R.c.io == 'f64' else 2e-5
  for name, ref in (('unw_sg', sg), ('unw_gp', gp), ('unw_obs', ob)): R.pin(what, name, can[name], np.reshape(ref, -1), tol)


def forward_forms(R):
  be, c = R.be, R.c
  step = lambda ab: dict(zip(STEP_NAMES, be.step(*R.a, absent=ab, **R.kw)))
  can = step(())
  if R.oracle: _pin_step(R, 'step', can)
  R.sweep('step', step, ('err', 'err_ext', 'info'), can)
  if c.cov in ('static', 'perstate'):      # ONE error kernel whatever the covariances (dgp_host.h kernel_group): static and per-state epsilons
    ev = lambda ab: dict(zip(EVAL_NAMES, be.eval_errors(*R.a, absent=ab, **R.kw)))
    can_e = ev(())
    if R.oracle:
      R.pin('eval_errors', 'err', can_e['err'], can['err'], PC.TOL_ERR[c.io]); R.pin('eval_errors', 'err_ext', can_e['err_ext'], can['err_ext'], PC.TOL_ERR[c.io])
      _pin_unw(R, 'eval_errors', can_e, R.th)
    R.sweep('eval_errors', ev, EVAL_NAMES, can_e)
    nog = lambda ab: dict(zip(EVAL_NAMES, be.eval_errors(R.p, R.th, R.start, R.goal, None, absent=ab, **R.kw)))      # sdf = NULL: the grid-free errors
    can_rm = R.rowmajor(lambda: ev(()))
    if R.oracle and c.tiled: _pin_unw(R, 'eval_errors (row-major)', can_rm, R.th)
    for ab in ((), ('unw_sg',), ('unw_gp',)): R.compare('eval_errors sdf=NULL NULL %s' % ','.join(ab), nog(ab), can_rm)
  return can


def _grad_opt(R, with_sdf=True):
  c = R.c
  return ['g_th', 'g_start', 'g_goal'] + (['g_sdf'] if with_sdf else []) + (['g_qc_inv'] if R.qc is not None else []) + (['g_obs_w'] if R.ow is not None else []) + \
         (['g_eps'] if R.eps is not None else [])


def _production(opt):
  """PlanLayer's two patterns: a learned-covariance loop (no g_th, g_start, g_goal, g_sdf) and a TBPTT link (g_th alone)"""
  return [tuple(x for x in opt if x in ('g_th', 'g_start', 'g_goal', 'g_sdf')), tuple(x for x in opt if x != 'g_th')]


def backward_forms(R):
  be, c, io = R.be, R.c, R.c.io
  B, n, d = c.B, c.n, 2 * c.dof
  dth = be.step(*R.a, **R.kw)[0]
  gbar = PC.rnd(R.rs.randn(B, n, d), io); gext = PC.rnd(R.rs.randn(B), io)
  bw = lambda ab, gd=gbar, ge=gext: R.grads(be.backward(*R.a, dth, gd, ge, absent=ab, **R.gm, **R.kw))
  can = bw(())
  if R.pin16:
    from oracle import autograd_torch as AT
    g_o = AT.step_gradients(*R.a, gbar, gext, qc=R.okw['qc'], ow=R.ow, eps=R.eps, q_full=R.q_full)
    tol = 1e-6 if io == 'f64' else 2e-3 * F32_GRAD_SCALE
    for key in ('th', 'start', 'goal', 'sdf', 'qc', 'ow', 'eps'):
      if can[key] is None: continue
      a_ = can[key].sum(0, keepdims=True) if key == 'sdf' and c.grid != 'per' else can[key]
      R.pin('step backward', key, a_, g_o[key], tol, scale=g_o['th'] if key == 'sdf' else None)
  opt = _grad_opt(R)
  R.sweep('step backward', bw, opt, can, extra=_production(opt))
  # a NULL cotangent == an explicit zero cotangent
  z, ze = np.zeros_like(gbar), np.zeros_like(gext)
  for ab, gd, ge in ((('g_dtheta',), z, gext), (('g_err_ext',), gbar, ze), (('g_dtheta', 'g_err_ext'), z, ze)):
    R.compare('step backward NULL %s vs zero' % ','.join(ab), bw(ab), bw((), gd, ge))
  if c.cov in ('static', 'static_diag', 'static_full', 'perstate'):      # dgp_eval_errors_backward runs the STATIC kernel of the configured Q_c_inv whatever the mode; perstate: g_eps
    ce, cs, cg, co = (PC.rnd(R.rs.randn(B), io) for _ in range(4))
    eb = lambda ab, cot=(ce, cs, cg, co): R.grads(be.eval_backward(*R.a, *cot, eps=R.eps, io=io, absent=ab, **R.gm))
    can_e = eb(())
    if R.pin16: _pin_eval_backward(R, can_e, (ce, cs, cg, co))
    opt_e = ['g_th', 'g_start', 'g_goal', 'g_sdf'] + (['g_eps'] if R.eps is not None else [])
    R.sweep('eval backward', eb, opt_e, can_e)
    zero = np.zeros(B)
    names = ('g_err_ext', 'g_unw_sg', 'g_unw_gp', 'g_unw_obs')
    for ab in null_forms(names):      # (all four NULL: every gradient zero)
      R.compare('eval backward NULL %s vs zero' % ','.join(ab), eb(ab), eb((), tuple(zero if nm in ab else v for nm, v in zip(names, (ce, cs, cg, co)))))
    nog = lambda ab: R.grads(be.eval_backward(R.p, R.th, R.start, R.goal, None, None, cs, cg, None, eps=R.eps, io=io, absent=ab))      # sdf = NULL
    ref = R.rowmajor(lambda: eb(('g_sdf',), (zero, cs, cg, zero)))
    for ab in ((), ('g_th',), ('g_start', 'g_goal')): R.compare('eval backward sdf=NULL NULL %s' % ','.join(ab), nog(ab), ref)      # (zero cotangents on the grid's factors: g_eps zero either way)


def _pin_eval_backward(R, can, cot):
  """dgp_eval_errors_backward against torch autograd over the dense restatement's err_ext and unweighted errors"""
  import torch
  from oracle import autograd_torch as AT
  c = R.c
  B, n = c.B, c.n
  T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
  sq, so, se = R.p.static_covs(B)
  L = dict(th=T(R.th), start=T(R.start), goal=T(R.goal), sdf=T(R.sdf), eps=T(se if R.eps is None else R.eps.reshape(se.shape)))
  for v in L.values(): v.requires_grad_(True)
  sdfB = L['sdf'].expand(B, *L['sdf'].shape[1:]) if L['sdf'].shape[0] == 1 else L['sdf']
  _, _, eex = AT.plan_layer_forward(L['th'], L['start'], L['goal'], sdfB, T(sq), T(so), L['eps'], R.p)      # err_ext: the FIXED weights
  sg, gp, ob = AT.unweighted_errors(L['th'], L['start'], L['goal'], sdfB, L['eps'], R.p)
  loss = sum((T(v).reshape(-1) * e.reshape(-1)).sum() for v, e in zip(cot, (eex, sg, gp, ob)))
  gr = dict(zip(L.keys(), torch.autograd.grad(loss, list(L.values()), allow_unused=True)))
  tol = 1e-6 if c.io == 'f64' else 2e-3 * F32_GRAD_SCALE
  for key in ('th', 'start', 'goal', 'sdf', 'eps'):
    if can[key] is None: continue
    a_ = can[key].sum(0, keepdims=True) if key == 'sdf' and c.grid != 'per' else can[key]
    R.pin('eval backward', key, a_, gr[key].numpy(), tol, scale=gr['th'].numpy() if key == 'sdf' else None)


def loop_forms(R):
  be, c, io = R.be, R.c, R.c.io
  if c.cov == 'scalar': return      # (DGP_QC_SCALAR is a step-only mode)
  B, n, d = c.B, c.n, 2 * c.dof
  d0 = be.step(*R.a, **R.kw)[0]
  nrm = np.sort(np.sqrt((d0.reshape(B, -1) ** 2).sum(1)))
  tol_delta = 0.5 * (nrm[0] + nrm[1])      # the trajectory with the smallest first update stops after ONE iteration
  solve = lambda ab: dict(zip(SOLVE_NAMES, be.solve(*R.a, K, tol_delta, absent=ab, **R.kw)))
  can = solve(())
  its = can['iters']
  if not (its.min() == 1 and its.max() > 1): R.bad('fused loop', 'iters', its.tolist())
  if R.oracle:      # K chained oracle steps, each trajectory taken where the loop left it
    cur, fin, errs = R.th.copy(), R.th.copy(), []
    for k in range(K):
      d_k, e_k, x_k, _ = BT.gn_step(R.p, cur, R.start, R.goal, R.sdf, **R.okw)
      cur = cur + d_k; errs.append((e_k, x_k))
      fin[its == k + 1] = cur[its == k + 1]
    R.pin('fused loop', 'th_out', can['th_out'], fin, 1e-7 if io == 'f64' else 1e-5)
    R.pin('fused loop', 'err_hist[:, 0]', can['err_hist'][:, 0], errs[0][0], PC.TOL_ERR[io]); R.pin('fused loop', 'errext_hist[:, 0]', can['errext_hist'][:, 0], errs[0][1], PC.TOL_ERR[io])
    if can['info'].any(): R.bad('fused loop', 'info', 'set')
    for b in range(B):
      if not (np.all(np.isfinite(can['err_hist'][b, :its[b]])) and np.all(np.isnan(can['err_hist'][b, its[b]:]))): R.bad('fused loop', 'err_hist', 'rows written %s' % its[b])
  R.sweep('fused loop', solve, SOLVE_NAMES[1:], can)
  if c.cov not in ('static', 'static_diag', 'static_full') or n > 256: return      # (no th_hist beyond 256 states)
  # the traced loop (th_hist needs iters) and the chain backward
  TR = SOLVE_NAMES + ('th_hist',)
  valid = lambda f: tuple(f) + (('th_hist',) if 'iters' in f and 'th_hist' not in f else ())
  tr = lambda ab: dict(zip(TR, be.solve_traced(*R.a, K, tol_delta, io=io, absent=ab)))
  can_t = tr(())
  for nm in SOLVE_NAMES: R.compare('traced loop vs fused loop', {nm: can_t[nm]}, can)      # the history store does not touch the loop
  hist = can_t['th_hist']
  for b in range(B):
    if not (np.all(np.isfinite(hist[:its[b], b])) and np.all(np.isnan(hist[its[b]:, b])) and np.array_equal(hist[0, b], R.th[b])): R.bad('traced loop', 'th_hist', 'rows of trajectory %d' % b)
  R.sweep('traced loop', tr, TR[1:], can_t, valid=valid)
  gbar = PC.rnd(R.rs.randn(B, n, d), io)
  cb = lambda ab: R.grads(be.solve_backward(R.p, R.start, R.goal, R.sdf, K, hist, can_t['th_out'], its, gbar, io=io, absent=ab, **R.gm))
  can_c = cb(())
  if R.pin16:      # the chain of single-step backward launches (pinned in backward_forms) walked by hand through the history: test_hip_every_chain_backward_kernel's bounds
    tho = can_t['th_out']
    gcur = gbar.copy()
    acc = dict(start=np.zeros_like(R.start), goal=np.zeros_like(R.goal), sdf=np.zeros_like(R.sdf))
    for k in range(K - 1, -1, -1):
      on = its > k
      thk = np.where(on[:, None, None], np.nan_to_num(hist[k]), tho)
      nxt = np.where((its > k + 1)[:, None, None], np.nan_to_num(hist[min(k + 1, K - 1)]), tho)
      one = be.backward(R.p, thk, R.start, R.goal, R.sdf, nxt - thk, gcur * on[:, None, None], None, io=io, **R.gm)
      gcur = gcur + one['th'] * on[:, None, None]
      acc['start'] += one['start'] * on[:, None, None]; acc['goal'] += one['goal'] * on[:, None, None]; acc['sdf'] += one['sdf'].sum(0, keepdims=True) if c.grid != 'per' else one['sdf']
    for key, b_ in (('th', gcur), ('start', acc['start']), ('goal', acc['goal']), ('sdf', acc['sdf'])):
      a_ = can_c[key].sum(0, keepdims=True) if key == 'sdf' and c.grid != 'per' else can_c[key]
      R.pin('chain backward', key, a_, b_, ((1e-7 if key == 'sdf' else (5e-9 if c.cov == 'static_full' else 1e-9)) if io == 'f64' else 5e-3 * F32_GRAD_SCALE), scale=gcur if key == 'sdf' else None)
  R.sweep('chain backward', cb, ('g_th_init', 'g_start', 'g_goal', 'g_sdf'), can_c)


def errs_forms(R):
  """dgp_gn_step_errors (one launch without a forced shape, row-major grid, n <= 128 -- d = 6: not the general family; two otherwise) and its backward (d = 4: the
  fold prologue, one launch; d = 6: two launches through the workspace)"""
  be, c, io = R.be, R.c, R.c.io
  B, n, d = c.B, c.n, 2 * c.dof
  npdt = np.float64 if io == 'f64' else np.float32
  fw = lambda ab: dict(zip(ERRS_NAMES, be.step_errors(*R.a, absent=ab, **R.kw)))
  can = fw(())
  th_new = (R.th.astype(npdt) + can['dtheta'].astype(npdt)).astype(np.float64)      # the sum in the I/O type
  if R.oracle:
    _pin_step(R, 'step_errors', can)
    _pin_unw(R, 'step_errors', can, th_new)
  # unw_sg, unw_gp and unw_obs ALL NULL is dgp_gn_step by design (the header; dgp_host.h gn_step_errors: `errs` false -> MODE_STEP): where the errors run as the epilogue
  # of the twin kernels (one launch) that is ANOTHER kernel, a separate compilation that agrees to rounding only -- those forms are held to the pinned dgp_gn_step call
  can_step = dict(zip(STEP_NAMES, be.step(*R.a, **R.kw)))
  if R.oracle: _pin_step(R, 'step', can_step)
  R.sweep('step_errors', fw, ERRS_NAMES[1:], can, ref=lambda ab: can_step if all(nm in ab for nm in ERRS_NAMES[4:]) else can)
  gd = PC.rnd(R.rs.randn(B, n, d), io)
  ce, cs, cg, co = (PC.rnd(R.rs.randn(B), io) for _ in range(4))
  gm = R.gm
  bw = lambda ab, g_=gd, cot=(ce, cs, cg, co): R.grads(be.step_errors_backward(*R.a, can['dtheta'], g_, *cot, absent=ab, **gm, **R.kw))
  can_b = bw(())
  if R.pin16:      # the two pinned launches it fuses (test_hip_every_step_errors_kernel's bound): the errors' backward at th + dtheta, then the step's with that gradient joined to the dtheta cotangent
    h1 = be.eval_backward(R.p, th_new, R.start, R.goal, R.sdf, None, cs, cg, co, eps=R.eps, io=io, sdf_grad='none')
    h2 = be.backward(*R.a, can['dtheta'], (gd.astype(npdt) + h1['th'].astype(npdt)).astype(np.float64), ce, sdf_grad='none', **R.kw)
    want = dict(th=h2['th'] + h1['th'], start=h2['start'] + h1['start'], goal=h2['goal'] + h1['goal'], qc=h2['qc'], ow=h2['ow'], eps=None if R.eps is None else h2['eps'] + h1['eps'])
    for key, ref in want.items():
      if ref is not None: R.pin('step_errors backward', key, can_b[key], ref, 1e-7 if io == 'f64' else 2e-3 * F32_GRAD_SCALE)
  opt = _grad_opt(R) + ([] if c.dof == 3 else ['workspace'])      # (d = 6: the two launches need the workspace)
  R.sweep('step_errors backward', bw, opt, can_b, extra=_production(opt))
  z, zero = np.zeros_like(gd), np.zeros(B)
  names = ('g_err_ext', 'g_unw_sg', 'g_unw_gp', 'g_unw_obs')
  R.compare('step_errors backward NULL g_dtheta vs zero', bw(('g_dtheta',)), bw((), z))
  for ab in [(nm,) for nm in names] + [names[1:]]:
    if ab == names[1:] and c.grid == 'per': continue      # (no unweighted-error cotangent: ONE tap block instead of two -- the sparse arrays change shape by design)
    R.compare('step_errors backward NULL %s vs zero' % ','.join(ab), bw(ab), bw((), gd, tuple(zero if nm in ab else v for nm, v in zip(names, (ce, cs, cg, co)))))


FORMS = dict(forward=forward_forms, backward=backward_forms, loop=loop_forms, errs=errs_forms)


def run_config(be, c, groups, fails, oracle=True):
  """every call form of the groups' entry points on configuration c; failures are appended to `fails` as (configuration, form, output, what).  -> comparisons made"""
  old = (be.guard, be.sdf_tiled, be.misalign)
  be.guard, be.sdf_tiled, be.misalign = True, c.tiled, False
  try:
    with forced_shape(c.shape):
      R = Run(be, c, fails, oracle)
      for g in groups: FORMS[g](R)
      return R.compared
  finally:
    be.guard, be.sdf_tiled, be.misalign = old


def long_configs(io):
  """the loop kernels of gn_long.h (n = 257: the ND_LONG pairs of parity_cases) -- run the groups 'forward', 'backward' and 'loop' on them: step, error kernel, fused
  loop, step backward, eval backward.  No scaled family, traced loop, chain backward, step-errors, sparse or float64 grid gradient there (the header)."""
  return [Cfg(dof, io, None, n, cov, grid='dense', B=3) for dof, n, cov, _ in PC.ND_LONG]
