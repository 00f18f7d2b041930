"""numpy fp64 restatement of dgp_heading_lift (include/dgpmp2_hip.h), written independently of the kernel: the tangents and their forward fill as a plain loop, the
turns, the prefix sum psi in the header's association order (SCAN, restated here), the end headings with this file's own use of Philox4x32-10, the blend, the
velocities and info.  numpy's element-wise + - * / are IEEE binary64 and never contract a * b + c, so with SUPPLIED turns this file and the kernel agree bit for bit
(tests/test_hip_heading.py); generated turns go through this platform's atan2 and agree to a few ulp.  tests/test_heading_oracle.py holds this file against the
reference's own straight_line_trajb (fixture g14_heading_lift) and against the invariants the rule was made for."""
import numpy as np

from problems_oracle import philox4x32_10

PI, TWO_PI = 3.141592653589793, 6.283185307179586
LINEAR, TANGENT = 0, 1                      # DGP_HEADING_*
SUPPLIED, END_TANGENT, RANDOM = 0, 1, 2     # DGP_END_*
KEEP, DIFF = 0, 1                           # DGP_VEL_*
HEADING = {'linear': LINEAR, 'tangent': TANGENT}
END = {'supplied': SUPPLIED, 'tangent': END_TANGENT, 'random': RANDOM}
VEL = {'keep': KEEP, 'diff': DIFF}
ALL_DEGENERATE, FILLED, SHARP_TURN, NON_FINITE = 1, 2, 4, 8      # info bits
HEADING_STREAM = 2


def rnd(a, io): return np.asarray(a, dtype=np.float32).astype(np.float64) if io == 'f32' else np.asarray(a, dtype=np.float64)


def wrap(a): return a - TWO_PI * np.rint(a / TWO_PI)


def scan(e):
  """the header's SCAN along the last axis: Hillis-Steele inside blocks of 64 indices, then the carry of the block before added to every element"""
  e = np.array(e, dtype=np.float64)
  n = e.shape[-1]
  for k0 in range(0, n, 64):
    blk = e[..., k0:k0 + 64]
    off = 1
    while off < 64:
      if off < blk.shape[-1]:
        new = blk.copy()
        new[..., off:] = blk[..., :-off] + blk[..., off:]
        blk[...] = new
      off *= 2
    if k0 > 0: blk[...] = e[..., k0 - 1:k0] + blk
  return e


def random_ends(seed, problem):
  """-> theta_s, theta_g of DGP_END_RANDOM for one problem"""
  w = philox4x32_10((problem & 0xffffffff, (problem >> 32) & 0xffffffff, 0, HEADING_STREAM), (seed & 0xffffffff, (seed >> 32) & 0xffffffff))
  u0 = float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53
  u1 = float(((w[2] << 32) | w[3]) >> 11) * 2.0 ** -53
  return (-PI) + u0 * TWO_PI, (-PI) + u1 * TWO_PI


def tangents(x, y):
  """-> t (n,2) unfilled, u (n,2) forward-filled, degenerate (n,) bool, any_valid"""
  n = x.shape[0]
  N = n - 1
  i = np.arange(n)
  lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, N)
  t = np.stack([x[hi] - x[lo], y[hi] - y[lo]], axis=1)
  deg = ((t[:, 0] == 0.0) & (t[:, 1] == 0.0)) | ~np.isfinite(t[:, 0]) | ~np.isfinite(t[:, 1])
  valid = np.flatnonzero(~deg)
  u = np.empty_like(t)
  if valid.size == 0:
    u[:] = (1.0, 0.0)
  else:
    last = t[valid[0]]      # leading degenerate rows: the first non-degenerate tangent
    for r in range(n):
      if not deg[r]: last = t[r]
      u[r] = last
  return t, u, deg, valid.size > 0, lo, hi


def turns_of(u):
  n = u.shape[0]
  turn = np.empty(n)
  turn[0] = np.arctan2(u[0, 1], u[0, 0])
  c = u[:-1, 0] * u[1:, 1] - u[:-1, 1] * u[1:, 0]
  c = np.where(c == 0.0, 0.0, c)
  d = u[:-1, 0] * u[1:, 0] + u[:-1, 1] * u[1:, 1]
  turn[1:] = np.arctan2(c, d)
  return turn


def lift_one(th2, total_time_sec, heading, start_end, goal_end, velocity, blend, ths, thg, turns_in):
  """one trajectory: th2 (n,4) float64 (holding io-rounded values), ths / thg floats (supplied or random; ignored for a TANGENT end) -> th (n,6) UNROUNDED doubles
  (columns 0, 1 and, for KEEP, 3, 4 are copies), turns (n,), info"""
  n = th2.shape[0]
  N = n - 1
  x, y = th2[:, 0], th2[:, 1]
  delta = total_time_sec / float(N)
  i = np.arange(n)
  t, u, deg, any_valid, lo, hi = tangents(x, y)
  info = 0
  if not (np.isfinite(x).all() and np.isfinite(y).all()): info |= NON_FINITE
  if start_end == SUPPLIED and not np.isfinite(ths): info |= NON_FINITE
  if goal_end == SUPPLIED and not np.isfinite(thg): info |= NON_FINITE
  th = np.zeros((n, 6))
  th[:, 0], th[:, 1] = x, y
  if heading == TANGENT:
    if not any_valid: info |= ALL_DEGENERATE
    if deg.any(): info |= FILLED
    turn = np.array(turns_in, dtype=np.float64) if turns_in is not None else turns_of(u)
    if (np.abs(turn[1:]) > PI / 2.0).any(): info |= SHARP_TURN
    e = turn.copy()
    e[0] = 0.0
    psi = scan(e)
    if start_end == END_TANGENT: theta_s, e_s = turn[0], 0.0
    else: theta_s, e_s = ths, wrap(ths - turn[0])
    base = theta_s - e_s
    phi = base + psi
    e_g = 0.0 if goal_end == END_TANGENT else wrap(thg - phi[N])
    ws = np.maximum(0.0, 1.0 - i.astype(np.float64) / float(blend))
    wg = np.maximum(0.0, 1.0 - (N - i).astype(np.float64) / float(blend))
    theta = (phi + ws * e_s) + wg * e_g
    theta[0] = theta_s
    theta[N] = phi[N] + e_g
    w0, wN = theta[0], theta[N]
  else:
    turn = np.zeros(n)
    theta = ths * (N - i).astype(np.float64) * 1.0 / float(N) * 1.0 + thg * i.astype(np.float64) * 1.0 / float(N) * 1.0
    w0, wN = ths, thg
  th[:, 2] = theta
  if velocity == DIFF:
    den = (hi - lo).astype(np.float64) * delta
    th[:, 3], th[:, 4] = t[:, 0] / den, t[:, 1] / den
    th[:, 5] = (theta[hi] - theta[lo]) / den
  else:
    th[:, 3], th[:, 4] = th2[:, 2], th2[:, 3]
    th[:, 5] = (wN - w0) / total_time_sec * 1.0
  return th, turn, info


def run(th2, total_time_sec, heading='tangent', ends='supplied', velocity='diff', blend=1, start_heading=None, goal_heading=None, turns=None, seed=0, first_problem=0,
        io='f64'):
  """th2 (B,n,4) holding io-rounded values -> start, goal (B,1,6), th (B,n,6) as float64 holding io-rounded values, turns (B,n) float64, info (B) int32"""
  th2 = np.asarray(th2, dtype=np.float64)
  B, n = th2.shape[:2]
  se, ge = (END[ends], END[ends]) if isinstance(ends, str) else (END[ends[0]], END[ends[1]])
  hm, vm = HEADING[heading], VEL[velocity]
  if hm == LINEAR and END_TANGENT in (se, ge): raise ValueError('tangent ends need tangent headings')
  if not 1 <= blend <= n - 1: raise ValueError('blend outside 1 .. N')
  th, start, goal = np.zeros((B, n, 6)), np.zeros((B, 1, 6)), np.zeros((B, 1, 6))
  turn, info = np.zeros((B, n)), np.zeros(B, np.int32)
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    for b in range(B):
      r_s, r_g = random_ends(seed, first_problem + b)
      ths = {SUPPLIED: None if start_heading is None else float(start_heading[b]), END_TANGENT: 0.0, RANDOM: r_s}[se]
      thg = {SUPPLIED: None if goal_heading is None else float(goal_heading[b]), END_TANGENT: 0.0, RANDOM: r_g}[ge]
      if ths is None or thg is None: raise ValueError('supplied ends need their arrays')
      t, turn[b], info[b] = lift_one(th2[b], float(total_time_sec), hm, se, ge, vm, int(blend), ths, thg, None if turns is None else turns[b])
      th[b] = rnd(t, io)
      th[b, :, :2] = th2[b, :, :2]      # bit for bit (a NaN's payload included)
      if vm == KEEP: th[b, :, 3:5] = th2[b, :, 2:4]
      start[b, 0, :3], goal[b, 0, :3] = th[b, 0, :3], th[b, n - 1, :3]
  return start, goal, th, turn, info
