"""Callers' helpers of the planner API, restated for torch tensors on any device.
Reference: diff_gpmp2/utils/planner_utils.py (check_convergence :3-16, check_convergence_batch :18-36,
straight_line_traj :38-45, straight_line_trajb :47-56, path_to_traj_avg_vel :60-71, smoothness_metrics :75-90,
collision_metrics :92-102).  The two metrics functions score ONE trajectory on the host side, like the reference; DiffGPMP2Planner.trajectory_metrics
scores a whole batch in one launch (dgp_traj_metrics) with the same definitions."""
import torch


def check_convergence(dtheta, j, err_delta, tol_err, tol_delta, max_iters, method='gauss_newton', verbose=False):
  """True when ||dtheta||_F < tol_delta or j >= max_iters (the err_delta / 'error increased' criteria are commented
  out in the reference, planner_utils.py:7-15, and stay inactive here)."""
  nrm = torch.norm(dtheta)
  if nrm < tol_delta:
    if verbose: print('Update got too small at iter %d: %f' % (j, nrm))
    return True
  if j >= max_iters:
    if verbose: print('Max iters done')
    return True
  return False


def check_convergence_batch(dthetab, j, err_delta, tol_err, tol_delta, max_iters, method='gauss_newton', device=None):
  """Per-sample convergence mask (B,1,1).  As in the reference (planner_utils.py:24-27) the second torch.where overwrites the
  first, so only the err_delta criterion survives: int64 ones/zeros from torch.where, or -- once j >= max_iters -- all ones
  as uint8 (the reference's torch.ones(...).byte(), created on the CPU whatever `device` says; here on dthetab's device)."""
  B = dthetab.shape[0]
  dev = dthetab.device if device is None else device
  err_delta_norm = torch.norm(err_delta.reshape(B, -1), dim=1, p=2)
  conv = torch.where(err_delta_norm < tol_err, torch.tensor(1, device=dev), torch.tensor(0, device=dev))
  if j >= max_iters:
    conv = torch.ones(B, 1, 1, dtype=torch.uint8, device=dthetab.device)
  return conv.view(B, 1, 1)


def straight_line_traj(start_conf, goal_conf, traj_time, num_steps, dof, device=None):
  """(1,dof) start/goal configurations -> (num_steps+1, 2*dof) constant-velocity straight line."""
  return straight_line_trajb(start_conf.reshape(1, 1, -1), goal_conf.reshape(1, 1, -1), traj_time, num_steps, dof, device)[0]


def straight_line_trajb(start_confb, goal_confb, traj_time, num_steps, dof, device=None):
  """(B,1,dof) start/goal configurations -> (B, num_steps+1, 2*dof).  Position i is
  start*(num_steps-i)/num_steps + goal*i/num_steps evaluated in the reference's operation order; velocity is the
  average velocity (goal-start)/traj_time at every state."""
  num_steps = int(num_steps)
  B = start_confb.shape[0]
  dev = start_confb.device if device is None else device
  s = start_confb[:, 0, 0:dof].to(dev); g = goal_confb[:, 0, 0:dof].to(dev)
  i = torch.arange(num_steps + 1, device=dev, dtype=s.dtype).view(1, -1, 1)
  pos = s.unsqueeze(1) * (num_steps - i) * 1.0 / num_steps * 1.0 + g.unsqueeze(1) * i * 1.0 / num_steps * 1.0
  vel = ((goal_confb.to(dev) - start_confb.to(dev)) / traj_time * 1.0)[:, :, 0:dof].expand(B, num_steps + 1, dof)
  return torch.cat((pos, vel), dim=-1).contiguous()


def path_to_traj_avg_vel(path, traj_time, dof, device=None):
  """A list of len(path) configurations -> (len(path), 2*dof): the path's positions, every velocity the average velocity
  (path[-1] - path[0]) / traj_time.  As the reference, the result is torch.zeros' default dtype."""
  num_steps = len(path)
  path = torch.stack([torch.as_tensor(q) for q in path])
  th_init = torch.zeros((num_steps, 2 * dof), device=device if device is not None else torch.device('cpu'))
  avg_vel = (path[-1] - path[0]) / traj_time * 1.0
  th_init[:, 0:dof] = path[:, 0:dof]
  th_init[:, dof:] = avg_vel
  return th_init


def smoothness_metrics(traj, total_time_sec, total_time_step):
  """traj (n, d) -> (avg_vel, avg_acc, avg_jerk), 0-d tensors: means of the row 2-norms of traj[:, 2:], of its first differences / total_time_step
  and of its second differences / total_time_step^2.  As in the reference the slice is 2: whatever dof (d = 6: theta, vx, vy, omega) and the divisor is
  the step COUNT, not dt; total_time_sec is unused."""
  tail = traj[:, 2:]
  d1 = tail[1:] - tail[:-1]
  d2 = d1[1:] - d1[:-1]
  mean_row_norm = lambda rows: torch.mean(torch.norm(rows, p=2, dim=1))
  return mean_row_norm(tail), mean_row_norm(d1 / total_time_step * 1.0), mean_row_norm(d2 / (total_time_step ** 2.0))


def collision_metrics(traj, obs_error, total_time_sec, total_time_step):
  """obs_error: the raw obstacle-factor errors of ONE trajectory, first dimension = state -> (in_coll, avg_penetration, max_penetration, coll_intensity) over
  the interior states (first and last dropped).  num_penetrating = numel(nonzero(obs_error)) / 2 as in the reference: with the (n,1,1) tensor the reference's
  callers pass (obs_error[0] of ObstacleFactor.get_error) nonzero() has three columns and this is 1.5 x the number of penetrating states -- coll_intensity
  inherits the factor; with an (n,1) tensor it is the count itself.  in_coll is a Python bool, coll_intensity a Python float (torch.numel returns an int)."""
  interior = obs_error[1:-1]
  num_penetrating = torch.nonzero(interior).numel() / 2
  step_sec = total_time_sec * 1.0 / total_time_step * 1.0
  return num_penetrating > 0, interior.mean(), interior.max(), (num_penetrating * step_sec) / total_time_sec * 1.0


def gp_interpolate_times(total_time_sec, total_time_step, num_inter, dtype=torch.float64, device=None):
  """(N_d,) query times of the dense trajectory: dense index m = i (K + 1) + j lies at i dt + j dt / (K + 1), dt = total_time_sec / total_time_step."""
  K1 = int(num_inter) + 1
  dt = total_time_sec * 1.0 / total_time_step * 1.0
  m = torch.arange(int(total_time_step) * K1 + 1, device=device)
  return (m // K1).to(dtype) * dt + (m % K1).to(dtype) * dt / K1


def gp_interpolate_traj(trajb, total_time_sec, total_time_step, num_inter):
  """(B, n, d) support states -> (B, N_d, d) dense trajectory, N_d = (n - 1)(num_inter + 1) + 1: GPMP2's GP interpolation, the posterior mean of the
  constant-velocity prior between two support states (Lambda(tau) theta_i + Psi(tau) theta_{i+1}; Q_c cancels).  The documented mirror of dgp_gp_interpolate
  (include/dgpmp2_hip.h states the closed form) as plain batched torch ops on any device, in trajb's dtype: the reference reads the keys 'total_check_step' /
  'use_gp_inter' (gpmp2_planner.py:29-41) and never interpolates.  Offset-0 rows are the support states themselves; the heading of the dof 3 robot is
  interpolated like any other column.  DiffGPMP2Planner.interpolate does the same (in fp64, with the collision check of every dense state) in one launch."""
  B, n, d = trajb.shape
  if n != int(total_time_step) + 1: raise ValueError('trajb has %d states for total_time_step %d' % (n, total_time_step))
  dof, K1 = d // 2, int(num_inter) + 1
  if K1 < 1: raise ValueError('num_inter must be >= 0')
  dt = total_time_sec * 1.0 / total_time_step * 1.0
  if K1 == 1: return trajb.clone()
  s = (torch.arange(K1, device=trajb.device, dtype=trajb.dtype) / K1).view(1, 1, K1, 1)
  s2 = s * s
  s3 = s2 * s
  x0, v0, x1, v1 = (t.unsqueeze(2) for t in (trajb[:, :-1, :dof], trajb[:, :-1, dof:], trajb[:, 1:, :dof], trajb[:, 1:, dof:]))
  pos = (((1.0 - 3.0 * s2) + 2.0 * s3) * x0 + (dt * ((s - 2.0 * s2) + s3)) * v0 + (3.0 * s2 - 2.0 * s3) * x1) + (dt * (s3 - s2)) * v1
  b2 = (6.0 * (s - s2)) / dt
  vel = ((-b2) * x0 + ((1.0 - 4.0 * s) + 3.0 * s2) * v0 + b2 * x1) + (3.0 * s2 - 2.0 * s) * v1
  out = torch.cat((pos, vel), dim=-1)                       # (B, n - 1, K1, d)
  out[:, :, 0] = trajb[:, :-1]                              # offset 0: the support state itself, no arithmetic
  return torch.cat((out.reshape(B, (n - 1) * K1, d), trajb[:, -1:]), dim=1)


def gp_prior_samples_torch(startb, goalb, noise, total_time_sec, total_time_step, Q_c_inv, K_s, K_g, mean=None, scale=1.0):
  """Trajectory samples from the GP prior between startb and goalb (B,1,d) from the standard normals noise (B,S,n+1,d) -> (B,S,n,d): the documented mirror of
  dgp_prior_samples (include/dgpmp2_hip.h states the construction) as plain batched torch ops on any device, in noise's dtype.  The unconditioned
  constant-velocity chain from the start prior (row 0 of the noise; rows 1 .. n-1 drive the intervals) as two cumulative sums, one noisy observation of its last
  state (row n), and Matheron's rule: xi_k = x_k - W_k y has exactly the covariance (A^T K^-1 A)^-1 of the planner's start, goal and GP factors.  mean (B,n,d) or
  None: the prior mean Phi(t_k) start + W_k (goal - Phi(T) start); scale multiplies xi.  DiffGPMP2Planner.sample_prior does the same in one launch, generating the
  normals on the device; the kernel's sums associate differently, so the two agree to rounding, not bit for bit."""
  B, S, n1, d = noise.shape
  n, dof = n1 - 1, d // 2
  if n != int(total_time_step) + 1: raise ValueError('noise has %d rows for total_time_step %d (n + 1 rows are needed)' % (n1, total_time_step))
  dev, dt_ = noise.device, noise.dtype
  f = lambda v: float(v.item()) if torch.is_tensor(v) else float(v)
  ks, kg, T = f(K_s), f(K_g), f(total_time_sec)
  dt = T * 1.0 / total_time_step * 1.0
  qc = torch.linalg.inv(torch.as_tensor(Q_c_inv, dtype=torch.float64, device='cpu'))
  lc = torch.linalg.cholesky(qc)
  t = torch.arange(n, dtype=torch.float64) * dt                                     # (n,)
  t_end = float(t[-1])
  I = torch.eye(dof, dtype=torch.float64)

  def P(tt):      # (..., d, d): K_s^2 Phi Phi^T + Q(t)
    tt = tt.reshape(-1, 1, 1)
    pp = ks * ks * (1.0 + tt * tt) * I + tt ** 3 / 3.0 * qc
    pv = ks * ks * tt * I + tt ** 2 / 2.0 * qc
    vv = ks * ks * I + tt * qc
    return torch.cat((torch.cat((pp, pv), -1), torch.cat((pv, vv), -1)), -2)
  Sinv = torch.linalg.inv(P(torch.tensor([t_end], dtype=torch.float64))[0] + kg * kg * torch.eye(d, dtype=torch.float64))
  tau = (t_end - t).reshape(-1, 1, 1)
  Z = torch.zeros(n, dof, dof, dtype=torch.float64)
  phi_t = torch.cat((torch.cat((I.expand(n, dof, dof), Z), -1), torch.cat((tau * I, I.expand(n, dof, dof)), -1)), -2)      # Phi(t_end - t_k)^T
  W = (P(t) @ phi_t @ Sinv).to(device=dev, dtype=dt_)                                # (n, d, d)
  lc, t = lc.to(device=dev, dtype=dt_), t.to(device=dev, dtype=dt_)
  z0, zi, zg = noise[:, :, 0], noise[:, :, 1:n], noise[:, :, n]
  lu, lw = zi[..., :dof] @ lc.T, zi[..., dof:] @ lc.T                                # (B,S,n-1,dof)
  wp = (dt ** 1.5 / 3.0 ** 0.5) * lu
  wv = (3.0 ** 0.5 / 2.0 * dt ** 0.5) * lu + (dt ** 0.5 / 2.0) * lw
  v = torch.cumsum(torch.cat((ks * z0[..., None, dof:], wv), 2), 2)                  # (B,S,n,dof)
  p = torch.cumsum(torch.cat((ks * z0[..., None, :dof], wp + dt * v[:, :, :-1]), 2), 2)
  x = torch.cat((p, v), -1)
  y = x[:, :, -1] + kg * zg                                                          # (B,S,d)
  xi = x - torch.einsum('kij,bsj->bski', W, y)
  if mean is None:
    st, go = startb[:, 0].to(dt_), goalb[:, 0].to(dt_)
    sp, sv = st[:, :dof], st[:, dof:]
    r0 = torch.cat((go[:, :dof] - (sp + t_end * sv), go[:, dof:] - sv), -1)
    m = torch.cat((sp[:, None] + t[None, :, None] * sv[:, None], sv[:, None].expand(B, n, dof)), -1) + torch.einsum('kij,bj->bki', W, r0)
  else:
    m = mean.to(dt_)
  return m[:, None] + scale * xi


_HL_PI, _HL_TWO_PI = 3.141592653589793, 6.283185307179586
_HL_HEADING, _HL_END, _HL_VEL = {'linear': 0, 'tangent': 1}, {'supplied': 0, 'tangent': 1, 'random': 2}, {'keep': 0, 'diff': 1}


def _hl_scan(e):
  """dgp_prior_samples' SCAN along the last axis (include/dgpmp2_hip.h): Hillis-Steele steps inside blocks of 64 indices, then the finished last value of the block
  before added to every element of a block"""
  e = e.clone()
  n = e.shape[-1]
  for k0 in range(0, n, 64):
    blk = e[..., k0:k0 + 64]
    off = 1
    while off < 64:
      if off < blk.shape[-1]:
        new = blk.clone()
        new[..., off:] = blk[..., :-off] + blk[..., off:]
        blk.copy_(new)
      off *= 2
    if k0 > 0: blk.copy_(e[..., k0 - 1:k0] + blk)
  return e


def _hl_random_ends(seed, problem):
  """theta_s, theta_g of DGP_END_RANDOM: one Philox4x32-10 block, counter (problem lo, problem hi, 0, 2), key (seed lo, seed hi)"""
  M = 0xffffffff
  c0, c1, c2, c3, k0, k1 = problem & M, (problem >> 32) & M, 0, 2, seed & M, (seed >> 32) & M
  for r in range(10):
    if r: k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
    c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M, (p0 >> 32) ^ c3 ^ k1, p0 & M
  u0, u1 = float(((c0 << 32) | c1) >> 11) * 2.0 ** -53, float(((c2 << 32) | c3) >> 11) * 2.0 ** -53
  return (-_HL_PI) + u0 * _HL_TWO_PI, (-_HL_PI) + u1 * _HL_TWO_PI


def heading_lift_torch(th2b, total_time_sec, start_heading=None, goal_heading=None, heading='tangent', ends='supplied', velocity='diff', blend=None, seed=0,
                       first_problem=0, turns=None):
  """Planar trajectories th2b (B,n,4) lifted to problems of the x-y-heading robot -> (startb (B,1,6), goalb (B,1,6), thb (B,n,6), turns (B,n) float64, info (B,)
  int32): the documented mirror of dgp_heading_lift (include/dgpmp2_hip.h states the rule) as batched torch ops on any device, the CPU included, computed in float64
  and rounded once to th2b's dtype.  heading 'tangent' | 'linear'; ends 'supplied' | 'tangent' | 'random' or a (start, goal) pair of those; velocity 'diff' | 'keep';
  blend default max(1, N // 4); start_heading / goal_heading (B,) for supplied ends; turns (B,n): the signed turns to use instead of atan2 of the tangents (what
  DiffGPMP2Planner.lift_headings(return_turns=True) returned) -- with them the result on the CPU equals the kernel's bit for bit (a device's torch kernels may
  contract a multiply-add: equal to rounding there), without them to the few ulp between two atan2."""
  B, n = int(th2b.shape[0]), int(th2b.shape[1])
  N = n - 1
  if blend is None: blend = max(1, N // 4)
  se, ge = (_HL_END[ends], _HL_END[ends]) if isinstance(ends, str) else (_HL_END[ends[0]], _HL_END[ends[1]])
  hm, vm = _HL_HEADING[heading], _HL_VEL[velocity]
  if hm == 0 and 1 in (se, ge): raise ValueError("ends='tangent' needs heading='tangent'")
  if not 1 <= int(blend) <= N: raise ValueError('blend must be in 1..%d, got %r' % (N, blend))
  dev, f64 = th2b.device, torch.float64
  T = float(total_time_sec)
  delta = T / float(N)
  p = th2b[..., :2].to(f64)
  x, y = p[..., 0], p[..., 1]
  idx = torch.arange(n, device=dev)
  lo, hi = torch.clamp(idx - 1, min=0), torch.clamp(idx + 1, max=N)
  tx, ty = x[:, hi] - x[:, lo], y[:, hi] - y[:, lo]
  deg = ((tx == 0) & (ty == 0)) | ~torch.isfinite(tx) | ~torch.isfinite(ty)
  info = (~(torch.isfinite(x).all(1) & torch.isfinite(y).all(1))).to(torch.int32) * 8

  def end(mode, arr, which):
    if mode == 0:
      if arr is None: raise ValueError("ends='supplied' needs start_heading and goal_heading")
      return torch.as_tensor(arr, dtype=f64, device=dev).reshape(B)
    if mode == 2: return torch.tensor([_hl_random_ends(int(seed), int(first_problem) + b)[which] for b in range(B)], dtype=f64, device=dev)
    return torch.zeros(B, dtype=f64, device=dev)
  ths, thg = end(se, start_heading, 0), end(ge, goal_heading, 1)
  if se == 0: info = info | (~torch.isfinite(ths)).to(torch.int32) * 8
  if ge == 0: info = info | (~torch.isfinite(thg)).to(torch.int32) * 8
  fi = idx.to(f64)
  if hm == 1:
    # forward fill: the last valid index at or before each row, the first valid one for leading rows, (1, 0) without any
    last = torch.cummax(torch.where(deg, torch.full_like(idx, -1).expand(B, n), idx.expand(B, n)), dim=1)[0]
    any_valid = (~deg).any(1)
    first = torch.argmax((~deg).to(torch.int32), dim=1)
    src = torch.where(last >= 0, last, first[:, None].expand(B, n))
    ux, uy = torch.gather(tx, 1, src), torch.gather(ty, 1, src)
    ux = torch.where(any_valid[:, None], ux, torch.ones_like(ux))
    uy = torch.where(any_valid[:, None], uy, torch.zeros_like(uy))
    if turns is not None: turn = torch.as_tensor(turns, dtype=f64, device=dev).reshape(B, n)
    else:
      c = ux[:, :-1] * uy[:, 1:] - uy[:, :-1] * ux[:, 1:]
      c = torch.where(c == 0, torch.zeros_like(c), c)
      d = ux[:, :-1] * ux[:, 1:] + uy[:, :-1] * uy[:, 1:]
      turn = torch.cat((torch.atan2(uy[:, :1], ux[:, :1]), torch.atan2(c, d)), 1)
    info = info | (~any_valid).to(torch.int32) | deg.any(1).to(torch.int32) * 2 | (turn[:, 1:].abs() > _HL_PI / 2.0).any(1).to(torch.int32) * 4
    psi = _hl_scan(torch.cat((torch.zeros(B, 1, dtype=f64, device=dev), turn[:, 1:]), 1))
    wrap = lambda a: a - _HL_TWO_PI * torch.round(a / _HL_TWO_PI)
    theta_s = turn[:, 0] if se == 1 else ths
    e_s = torch.zeros_like(ths) if se == 1 else wrap(ths - turn[:, 0])
    base = theta_s - e_s
    phi = base[:, None] + psi
    e_g = torch.zeros_like(thg) if ge == 1 else wrap(thg - phi[:, N])
    ws = torch.clamp(1.0 - fi / float(blend), min=0.0)
    wg = torch.clamp(1.0 - (N - idx).to(f64) / float(blend), min=0.0)
    theta = (phi + ws[None] * e_s[:, None]) + wg[None] * e_g[:, None]
    theta[:, 0] = theta_s
    theta[:, N] = phi[:, N] + e_g
    w0, wN = theta[:, 0], theta[:, N]
  else:
    turn = torch.zeros(B, n, dtype=f64, device=dev)
    theta = ths[:, None] * (N - idx).to(f64)[None] * 1.0 / float(N) * 1.0 + thg[:, None] * fi[None] * 1.0 / float(N) * 1.0
    w0, wN = ths, thg
  thb = torch.empty(B, n, 6, dtype=th2b.dtype, device=dev)
  thb[..., :2] = th2b[..., :2]
  thb[..., 2] = theta.to(th2b.dtype)
  if vm == 1:
    den = (hi - lo).to(f64) * delta
    thb[..., 3], thb[..., 4] = (tx / den).to(th2b.dtype), (ty / den).to(th2b.dtype)
    thb[..., 5] = ((theta[:, hi] - theta[:, lo]) / den).to(th2b.dtype)
  else:
    thb[..., 3:5] = th2b[..., 2:4]
    thb[..., 5] = ((wN - w0) / T * 1.0).to(th2b.dtype)[:, None]
  zeros = torch.zeros(B, 1, 3, dtype=th2b.dtype, device=dev)
  return torch.cat((thb[:, :1, :3], zeros), -1), torch.cat((thb[:, N:, :3], zeros), -1), thb, turn, info


SEL_COLLIDING, SEL_OUTSIDE, SEL_NON_FINITE, SEL_EXCLUDED = 1, 2, 4, 8      # bits of dgp_select_samples' `status`
SELECT_NAMES = ('solved', 'num_accepted', 'best_index', 'best_score', 'best_max_penetration', 'best_status')      # columns of its problem summary


class SelectInfo(object):
  """What dgp_select_samples reports, device tensors (select_samples_torch: on thb's device): `best` (B,) int32 the chosen sample of every problem; `status` (B,S) int32
  of SEL_* bits and `order` (B,S) int32, all samples best first (None unless asked for); `sample_raw` (B,S,6) float64, the dense-check summary of every sample
  (columns _capi.DENSE_NAMES; None without grids); `raw` (B,6) float64 (columns SELECT_NAMES).  solved (bool: the chosen sample collides with nothing, stays inside
  the limits where that is required, is finite and not excluded), num_accepted (int64), best_score, best_max_penetration and the (B,S) bool views of `status`
  colliding, outside, non_finite, excluded are formed on access by one small torch op each."""
  __slots__ = ('best', 'status', 'order', 'sample_raw', 'raw')
  _COL = {name: i for i, name in enumerate(SELECT_NAMES)}
  _BITS = {'colliding': SEL_COLLIDING, 'outside': SEL_OUTSIDE, 'non_finite': SEL_NON_FINITE, 'excluded': SEL_EXCLUDED}

  def __init__(self, best, status, order, sample_raw, raw):
    self.best, self.status, self.order, self.sample_raw, self.raw = best, status, order, sample_raw, raw

  def __getattr__(self, name):
    if name in SelectInfo.__slots__: raise AttributeError(name)
    bit = self._BITS.get(name)
    if bit is not None: return (self.status & bit) != 0
    if name == 'solved': return self.raw[:, 0] != 0
    if name == 'num_accepted': return self.raw[:, 1].to(torch.int64)
    if name in ('best_score', 'best_max_penetration'): return self.raw[:, self._COL[name]]
    if name == 'best_status': return self.raw[:, 5].to(torch.int64)
    raise AttributeError(name)


def select_samples_torch(thb, sdfb=None, score=None, exclude=None, total_time_sec=10.0, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0), sphere_radius=0.0, num_inter=7, eps=0.0,
                         require_inside=True, env_index=None, sample_major=False):
  """Multi-start selection in plain torch ops on any device: the documented mirror of dgp_select_samples (include/dgpmp2_hip.h states the rule) and the definition
  of the long form -- per problem, the GP-interpolated dense check of each of its S optimised trajectories (gp_interpolate_traj, num_inter states per interval,
  bilinear lookup, hinge at eps + sphere_radius), the status bits, the tiers and the total order as a stable lexicographic sort, and the chosen trajectory by
  indexing.  thb (B,S,n,d) -- (S,B,n,d) with sample_major, like score and exclude; sdfb (B | 1,1,H,W) / (B | 1,H,W) / a TiledSdf: one grid per PROBLEM, one shared
  grid, or None (no collision check); env_index (B,): the grid of problem b.  The check runs in float64; its sums associate differently from the kernel's and its
  dense states agree with the kernel's to rounding, so the integer results are the kernel's and the penetrations agree to rounding.
  -> (th_best (B,n,d), SelectInfo) with status, order and sample_raw always present."""
  from .sdf_utils import _rowmajor_grids, bilinear_interpolate_torch
  th = thb.transpose(0, 1) if sample_major else thb
  B, S, n, d = th.shape
  dev = th.device
  pm = lambda t: (t.transpose(0, 1) if sample_major else t)
  sc = torch.zeros((B, S), dtype=torch.float64, device=dev) if score is None else pm(score).to(torch.float64)
  ex = torch.zeros((B, S), dtype=torch.bool, device=dev) if exclude is None else pm(exclude) != 0
  K = int(num_inter)
  dense = gp_interpolate_traj(th.reshape(B * S, n, d).to(torch.float64), total_time_sec, n - 1, K)      # (B S, N_d, d)
  nd = dense.shape[1]
  x, y = dense[:, :, 0], dense[:, :, 1]
  inside = (x >= float(x_lims[0])) & (x <= float(x_lims[1])) & (y >= float(y_lims[0])) & (y <= float(y_lims[1]))      # a NaN is outside
  outside = (~inside).any(1).view(B, S)
  sample_raw = None
  max_pen = torch.zeros((B, S), dtype=torch.float64, device=dev)
  colliding = torch.zeros((B, S), dtype=torch.bool, device=dev)
  if sdfb is not None:
    if nd < 3: raise ValueError('the collision check needs at least 3 dense states, got %d' % nd)
    g = _rowmajor_grids(sdfb).to(torch.float64)
    if env_index is not None: g = g.index_select(0, env_index.to(torch.int64))
    if g.shape[0] not in (1, B): raise ValueError('sdfb has %d grids for %d problems' % (g.shape[0], B))
    res = (float(x_lims[1]) - float(x_lims[0])) / g.shape[-1]
    dist = bilinear_interpolate_torch(g, dense[:, :, :2].reshape(B, S * nd, 2), res, x_lims, y_lims)[0].view(B, S, nd)
    tot = float(eps) + float(sphere_radius)
    cost = torch.where(dist <= tot, tot - dist, torch.zeros_like(dist))
    inner = cost[:, :, 1:-1]
    hit = inner != 0
    cnt = hit.sum(-1)
    nan = torch.isnan(inner)
    neg = torch.full_like(inner, float('-inf'))
    worst = torch.where(nan.any(-1), torch.argmax(nan.to(torch.int8), -1), torch.argmax(torch.where(nan, neg, inner), -1)) + 1
    max_pen = torch.where(nan.any(-1), torch.full_like(inner[..., 0], float('nan')), inner.max(-1)[0])
    first = torch.where(cnt > 0, torch.argmax(hit.to(torch.int8), -1) + 1, torch.full_like(cnt, -1))
    sample_raw = torch.stack(((cnt > 0).to(torch.float64), cnt.to(torch.float64), inner.mean(-1), max_pen, first.to(torch.float64), worst.to(torch.float64)), -1)
    colliding = cnt != 0
  non_finite = ~torch.isfinite(th.reshape(B, S, -1)).all(-1) | ~torch.isfinite(sc) | torch.isnan(max_pen)
  status = (colliding.to(torch.int32) * SEL_COLLIDING + outside.to(torch.int32) * SEL_OUTSIDE + non_finite.to(torch.int32) * SEL_NON_FINITE + ex.to(torch.int32) * SEL_EXCLUDED)
  two, one, zero = torch.full_like(status, 2), torch.full_like(status, 1), torch.zeros_like(status)
  tier = torch.where(non_finite | ex, two, torch.where(colliding | (outside if require_inside else torch.zeros_like(outside)), one, zero))
  # the total order as a stable lexicographic sort, least significant key first: (index,) score, penetration, tier
  zf = torch.zeros_like(sc)
  order = torch.arange(S, device=dev).expand(B, S)
  for key in (torch.where(tier < 2, sc, zf) + 0.0, torch.where(tier == 1, max_pen, zf) + 0.0, tier):      # (+ 0.0: -0.0 and 0.0 tie)
    order = order.gather(1, torch.sort(key.gather(1, order), dim=1, stable=True)[1])
  best = order[:, 0]
  rows = torch.arange(B, device=dev)
  raw = torch.stack(((tier[rows, best] == 0).to(torch.float64), (tier == 0).sum(1).to(torch.float64), best.to(torch.float64), sc[rows, best], max_pen[rows, best],
                     status[rows, best].to(torch.float64)), -1)
  return th[rows, best].clone(), SelectInfo(best.to(torch.int32), status, order.to(torch.int32), sample_raw, raw)
