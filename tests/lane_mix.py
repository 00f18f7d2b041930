"""Lane-mixed full-GPU batches (host only): the inputs of tests/test_hip_full_batch.py and tests/test_lane_mix.py.

The known failure class of this library is per-lane state that goes stale at a divergent join (DESIGN.md section 7,
profiles/r06_compiler_fault.md): a lane that skipped an `if` reloads a register / scratch slot that still holds an earlier
value, possibly an earlier WAVEFRONT's.  A test sees that only if (1) a SIMD runs more than one wavefront, so a slot can hold
what an earlier wavefront left there, and (2) the lanes of one trajectory, and the C states of one lane, take different sides
of the data-dependent branches.  make() builds batches with both properties by construction:

  * B = waves * TPW + TPW // 2 trajectories (TPW = 64 // LPT per wavefront; the last wavefront ragged), waves >= 2048 and by
    default enough for every SIMD of the GPU to run two of the kernel's wavefronts one after the other (default_waves);
  * in every wavefront, trajectory slot 0 carries a window of 8 consecutive states, lane-aligned, whose positions alternate
    between hinge-active points (inside the safety distance of an obstacle, outside the grid, in the last grid row, in the
    last grid column) and free points -- so the hinge decision differs between the lanes of one trajectory and, for C > 1,
    between the C states of one lane;
  * slot 1 leaves the grid (its goal lies beyond x = 5), slot 2 lies outside the grid entirely; every fourth wavefront of
    the one-trajectory shapes (LPT = 64) carries a leaving trajectory as well;
  * velocity limits (p.use_vel_limits): every third state of every trajectory moves faster than the limit, the rest
    at most 0.9 of it;
  * per-state modes: obstacle weights in [50, 2e4] with exact zeros, epsilons set 0.1 ... 0.4 above or below the state's
    obstacle distance (alternating by state), so the hinge decision of one lane is mixed by the epsilons as well;
  * one trajectory in every 64th wavefront with a NaN in th (nan_rows; not the mixed slot 0 unless LPT = 64);
  * 'scalar' modes (DGP_QC_SCALAR): per-state weights / epsilons as above and one scalar per GP factor, all squares of 11-bit numbers (exact in
    fp32); optionally one grid per trajectory of an odd size (grid=ODD_GRID).

Every number is rounded to fp32 (parity_cases.rnd), so the fp32 and the fp64 kernels see the same inputs.  The checks
(check_* below) return lists of failure strings naming the wavefront and the lane offset of the trajectory."""
import json
import os
import numpy as np
import parity_cases as PC
from oracle import gpmp2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = os.path.join(ROOT, 'dgpmp2_amd', 'lib', 'kernel_stats.json')
SHAPES = [(l, c) for l in (16, 32, 64) for c in (1, 2, 4)]
COVS = ['static', 'static_full', 'perstate', 'qfull']
# appended after COVS (configs): 'static_diag' -- a diagonal Q_c_inv that is not c I (QK_STATIC, block elimination with four states per lane, no Woodbury);
# 'scalar' -- DGP_QC_SCALAR (QK_SCALED, the learned mode diag_identity), per-state weights / epsilons as 'perstate', one scalar per GP factor scaling Q_c_inv = I
# ('scalar', 'scalar_raw': the same handed over as the learn module's raw output vector, squared by dgp_square_covariances) or Q_c_inv = QC_DIAG ('scalar_diag')
COVS_EXTRA = ['static_diag', 'scalar']
QC_DIAG = lambda dof: np.diag(1.0 + 0.5 * np.arange(dof))
ODD_GRID = (39, 41)           # the per-sample grids of odd_config: padding cells in the last 4 x 4 tile row and column of DGP_SDF_TILED4
CIRCLES = ((-2.0, -1.0, 1.0), (1.5, 2.0, 0.8), (0.0, 0.0, 0.7))
G = 40                        # grid cells: res = 10 / 40 = 0.25 exactly, last row y in (-5, -4.75], last column x in [4.75, 5)
MIN_WAVES = 2048              # 2 x 256 CUs x 4 SIMDs
MAX_STATES = 1 << 20          # cap of B * n: about 0.2 s of C oracle per step at 16 threads
SIMDS = 1024
MARGIN = 0.1                  # distance of every designed hinge / velocity decision from its threshold


def tpw(lpt): return 64 // lpt


def locate(b, lpt):
  """trajectory -> (wavefront, lane offset of its first lane)"""
  return b // tpw(lpt), (b % tpw(lpt)) * lpt


def default_waves(dof, lpt, c, n, stats_path=STATS):
  """Wavefronts per launch: two per SIMD at the kernel's resident waves per SIMD (the largest over the step / loop / backward kernels
  of this (dof, LPT, C) in the build's kernel_stats.json; 1 for the heavy spillers and when the file is absent), at least MIN_WAVES,
  at most MAX_STATES states."""
  occ = 1
  try:
    stats = json.load(open(stats_path))
    key = '<%d,%d,%d,' % (dof, lpt, c)
    occ = max([1] + [int(v.get('waves_per_simd', 1)) for k, v in stats.items() if isinstance(v, dict) and key in k and int(v.get('scratch_bytes_per_lane', 0)) == 0])
  except (OSError, ValueError):
    pass
  want = 2 * SIMDS * occ
  return int(max(MIN_WAVES, min(want, MAX_STATES // max(1, tpw(lpt) * n))))


def lookup(p, sdf, xy):
  """the oracle's bilinear distance at positions xy (..., 2), and whether the state lies in the grid's interior (no clamped index)"""
  sh = xy.shape[:-1]
  res = (p.x_lims[1] - p.x_lims[0]) / sdf.shape[-1]
  if sdf.shape[0] > 1:      # one grid per trajectory: xy (B, ..., 2)
    return O.bilinear_interpolate(sdf[:, 0], xy.reshape(sdf.shape[0], -1, 2), res, p.x_lims, p.y_lims)[0].reshape(sh)
  d, _ = O.bilinear_interpolate(np.broadcast_to(sdf[:, 0], (1,) + sdf.shape[-2:]), xy.reshape(1, -1, 2), res, p.x_lims, p.y_lims)
  return d.reshape(sh)


def hinge_active(p, sdf, th, eps=None):
  """(B, n) bool: the oracle's hinge decision dist <= eps + r (obstacle_cost.py:36)"""
  B, n = th.shape[:2]
  e = np.full((B, n), p.epsilon_dist) if eps is None else np.reshape(eps, (B, n))
  return lookup(p, sdf, th[:, :, :2]) <= e + p.radius


def out_of_grid(p, sdf, xy):
  """(...) bool: a bilinear index was clamped (outside the grid, or in its last row / column)"""
  res = (p.x_lims[1] - p.x_lims[0]) / sdf.shape[-1]
  px = -p.x_lims[0] / res + xy[..., 0] / res
  py = -p.y_lims[0] / res - xy[..., 1] / res
  H, W = sdf.shape[-2:]
  return ~((px >= 0) & (px < W - 1) & (py >= 0) & (py < H - 1))


def _points(rs, p, sdf, kind, k):
  """k positions of one kind: 'in' (hinge-active under the static epsilon), 'free' (inactive), 'outx' / 'outy' (outside the grid),
  'lastrow' / 'lastcol' (the degenerate last grid cell row / column)"""
  if kind in ('in', 'free'):
    out = np.empty((0, 2))
    thr = p.epsilon_dist + p.radius
    while len(out) < k:
      cand = rs.uniform(-4.5, 4.5, (8 * k + 16, 2))
      d = lookup(p, sdf, cand)
      ok = (d <= thr - MARGIN) if kind == 'in' else (d >= thr + MARGIN)
      out = np.concatenate([out, cand[ok & ~out_of_grid(p, sdf, cand)]])
    return out[:k]
  xy = rs.uniform(-4.5, 4.5, (k, 2))
  sgn = np.where(rs.rand(k) < 0.5, -1.0, 1.0)
  if kind == 'outx': xy[:, 0] = sgn * rs.uniform(5.2, 6.0, k)
  if kind == 'outy': xy[:, 1] = sgn * rs.uniform(5.2, 6.0, k)
  if kind == 'lastrow': xy[:, 1] = rs.uniform(-4.95, -4.8, k)
  if kind == 'lastcol': xy[:, 0] = rs.uniform(4.8, 4.95, k)
  return xy


WINDOW = ('in', 'free', 'outx', 'free', 'lastrow', 'free', 'lastcol', 'free')      # active / inactive alternate at every state


def window_start(b, n, c):
  """first state of trajectory b's mixed window: lane-aligned, the window inside [0, n)"""
  lanes = max(1, (n - len(WINDOW)) // c)
  return c * ((5 * b) % lanes)


class Batch(object):
  pass


def r11(a):
  """a rounded to 11 significant bits: its square, and the square times 1.5 (QC_DIAG), are exact in fp32 -- the squares of the 'scalar' modes and
  their dense blocks are the same numbers for fp32 and fp64 I/O"""
  m, e = np.frexp(np.asarray(a, np.float64))
  return np.ldexp(np.round(np.ldexp(m, 11)), e - 11)


def is_scalar(cov): return cov.startswith('scalar')


def make(dof, lpt, c, n, cov, vel=False, waves=None, seed=0, nan=True, io='f32', grid=None, reg=0.1):
  """-> Batch with p, th, start, goal, sdf, qc, ow, eps, q_full (harness.Backend's arguments), and B, lpt, c, waves, nan_rows, kinds.
  reg: the diagonal shift of Lambda = A^T K A + reg I (no other number of the batch depends on it; tests/spd_cases.py lowers it below zero).
  'scalar' modes: qc (B, n-1) the scalars, qc_dense (B, n-1, dof, dof) the blocks s_k Q_c_inv the oracles take, raw_out ('scalar_raw': the learn
  module's output vector [q_k, o_i, e_i] whose squares are qc, ow, eps) .  grid (H, W): one grid per trajectory, the shared one cropped to H x W
  (res = 10 / W) plus a constant offset per trajectory."""
  rs = np.random.RandomState(seed)
  d = 2 * dof
  T = tpw(lpt)
  waves = default_waves(dof, lpt, c, n) if waves is None else int(waves)
  B = waves * T + T // 2
  kw = dict(non_holonomic=True, K_d=0.1) if dof == 3 else {}
  if cov == 'static_full':
    A = rs.randn(dof, dof) * 0.3
    kw['Q_c_inv'] = np.eye(dof) + A @ A.T
  if cov in ('static_diag', 'scalar_diag'): kw['Q_c_inv'] = QC_DIAG(dof)
  p = O.OracleParams(dof=dof, total_time_step=n - 1, reg=reg, epsilon_dist=0.3, use_vel_limits=vel, **kw)
  sdf = O.circles_sdf(G, CIRCLES)[None, None] if grid is None else O.circles_sdf(max(grid), CIRCLES)[None, None, :grid[0], :grid[1]]
  slot = np.arange(B) % T
  wave = np.arange(B) // T
  kinds = np.full(B, 'line', dtype=object)
  kinds[slot == 0] = 'mixed'
  if T >= 2: kinds[slot == 1] = 'leave'
  if T >= 4: kinds[slot == 2] = 'outside'
  start = np.zeros((B, 1, d)); goal = np.zeros((B, 1, d))
  start[:, 0, :2] = rs.uniform(-4, 4, (B, 2)); goal[:, 0, :2] = rs.uniform(-4, 4, (B, 2))
  leave = (kinds == 'leave') | ((T == 1) & (wave % 4 == 1))
  goal[leave, 0, 0] = rs.uniform(6.0, 8.0, leave.sum())
  lv = kinds == 'leave'      # (away from the obstacles: a small first update, below the median one of the mixed trajectories)
  start[lv, 0, 0] = rs.uniform(3.0, 4.5, lv.sum()); start[lv, 0, 1] = rs.uniform(-4.5, -2.5, lv.sum())
  o = kinds == 'outside'
  start[o, 0, 0] = rs.uniform(5.5, 8.0, o.sum()); goal[o, 0, 0] = rs.uniform(5.5, 8.0, o.sum())
  if dof == 3:
    goal[:, 0, 2] = rs.uniform(-np.pi, np.pi, B)
    hd = np.arctan2(goal[lv, 0, 1] - start[lv, 0, 1], goal[lv, 0, 0] - start[lv, 0, 0])      # (leaving trajectories: heading along the line, no non-holonomic update)
    start[lv, 0, 2] = hd; goal[lv, 0, 2] = hd
  th = O.straight_line_trajb(start[:, :, :dof], goal[:, :, :dof], 10.0, n - 1, dof) + rs.randn(B, n, d) * 0.03
  mixed = np.nonzero(kinds == 'mixed')[0]
  side = np.where((np.arange(n)[None, :] + np.arange(B)[:, None]) % 2 == 0, 1.0, -1.0)      # per-state epsilons: + active, - inactive
  pos = {k: iter(_points(rs, p, sdf, k, len(mixed) * WINDOW.count('outx' if k == 'outy' else k))) for k in sorted(set(WINDOW) | {'outy'})}
  for b in mixed:
    g0 = window_start(b, n, c)
    for i, kind in enumerate(WINDOW[:n - g0]):
      if kind == 'outx' and b % 2: kind = 'outy'
      th[b, g0 + i, :2] = next(pos[kind])
      side[b, g0 + i] = -1.0 if kind == 'free' else 1.0
  if vel:      # velocity limits v_x = v_y = 1: every third state beyond them, the rest at most 0.9 (straight lines move at most 0.8 per second)
    v = np.clip(th[:, :, dof:dof + 2], -0.9, 0.9)
    fast = (np.arange(n)[None, :] + np.arange(B)[:, None]) % 3 == 0
    v[fast] = np.where(rs.rand(fast.sum(), 2) < 0.5, -1.0, 1.0) * rs.uniform(1.0 + MARGIN, 2.0, (fast.sum(), 2))
    th[:, :, dof:dof + 2] = v
  qc = ow = eps = qc_dense = raw_out = None; q_full = False
  if cov in ('perstate', 'qfull') or is_scalar(cov):
    ow = rs.uniform(50, 2e4, (B, n))
    ow[rs.rand(B, n) < 1.0 / 16] = 0.0
    dist = lookup(p, sdf, PC.rnd(th, io)[:, :, :2])
    eps = np.maximum(0.05, dist - p.radius + side * rs.uniform(MARGIN, 0.4, (B, n)))
    if cov == 'perstate':
      A = rs.randn(B, n - 1, dof, dof) * 0.2; qc = np.eye(dof) + A @ np.swapaxes(A, -1, -2)
    elif cov == 'qfull':
      A = rs.randn(B, n - 1, d, d) * 0.2; qc = (np.eye(d) + A @ np.swapaxes(A, -1, -2)) * 1.5; q_full = True
    else:      # the raw values q_k ~ U(0.3, 3), o_i, e_i at 11 bits: their squares, the scalars s_k = q_k^2 and the weights / epsilons, are exact in fp32
      q, o, e = r11(rs.uniform(0.3, 3.0, (B, n - 1))), r11(np.sqrt(ow)), r11(np.sqrt(eps))
      qc, ow, eps = q * q, o * o, e * e
      qc_dense = qc[:, :, None, None] * p.Q_c_inv
      sg = lambda a: a * np.where(rs.rand(*a.shape) < 0.5, -1.0, 1.0)      # (only the square enters)
      if cov == 'scalar_raw': raw_out = np.concatenate([sg(q), sg(o), e], 1)
  # the NaN trajectories: wavefronts 32, 96, 160, ... (the middle one of a batch of fewer than 33; wavefront 0 stays clean for the sampled checks), never
  # the designed mixed slot 0 where there is another one (the lane offset changes from one NaN wavefront to the next)
  nan_rows = np.array([w_ * T + (1 + (w_ // 64) % (T - 1) if T > 1 else 0) for w_ in range(min(32, waves // 2), waves, 64)], dtype=np.int64) if nan else np.zeros(0, np.int64)
  th_clean = th.copy()
  th[nan_rows, n // 2, 0] = np.nan
  if grid is not None:      # one grid per trajectory: the shared one plus a constant (|offset| < MARGIN / 2: every designed decision keeps its side)
    sdf = sdf + rs.uniform(-0.04, 0.04, (B, 1, 1, 1))
  r = lambda a: None if a is None else PC.rnd(a, io)
  bt = Batch()
  bt.qc_dense, bt.raw_out = qc_dense, raw_out
  bt.th_clean = r(th_clean)
  bt.p, bt.th, bt.start, bt.goal, bt.sdf, bt.qc, bt.ow, bt.eps, bt.q_full = p, r(th), r(start), r(goal), r(sdf), r(qc), r(ow), r(eps), q_full
  bt.dof, bt.B, bt.n, bt.lpt, bt.c, bt.cov, bt.waves, bt.nan_rows, bt.kinds = dof, B, n, lpt, c, cov, waves, nan_rows, kinds
  bt.tag = 'dof %d shape (%d,%d) n %d cov %s%s%s B %d (%d wavefronts)' % (dof, lpt, c, n, cov, ' vel' if vel else '', '' if grid is None else ' grids %dx%d' % grid, B, waves + (T > 1))
  return bt


def configs(dof):
  """the (lpt, c, n, cov, vel) configurations the full-batch test runs: every shape x covariance mode, exact fit for half of them and a
  ragged length for the other half, velocity limits (d = 4) in one covariance mode per shape.  Then every shape x COVS_EXTRA (the 36 above
  keep their order): 'static_diag' with velocity limits (d = 4) in the even shapes -- so (16,4) and (64,4) but not (32,4) --, 'scalar' with
  Q_c_inv = I in the even shapes (as the raw output vector in (16,4) and (64,1)) and Q_c_inv = QC_DIAG in the odd ones"""
  out = []
  for i, (lpt, c) in enumerate(SHAPES):
    for j, cov in enumerate(COVS):
      n = lpt * c if (i + j) % 2 == 0 else max(4, lpt * c - 3)
      out.append((lpt, c, n, cov, dof == 2 and j == i % len(COVS)))
  for i, (lpt, c) in enumerate(SHAPES):
    for j, cov in enumerate(COVS_EXTRA):
      n = lpt * c if (i + j) % 2 == 0 else max(4, lpt * c - 3)
      if cov == 'scalar': cov = 'scalar_diag' if i % 2 else ('scalar_raw' if i % 4 == 2 else 'scalar')
      out.append((lpt, c, n, cov, dof == 2 and cov == 'static_diag' and i % 2 == 0))
  return out


def config_waves(cov):
  """wavefronts of a configuration: the default for COVS, MIN_WAVES (two per SIMD at one wave per SIMD) for the modes of COVS_EXTRA"""
  return None if cov in COVS else MIN_WAVES


def odd_config(dof):
  """(lpt, c, n, cov, vel) of the configuration with per-sample grids of ODD_GRID (make(..., grid=ODD_GRID, waves=MIN_WAVES)): the tiled twins
  on padded tiles, the lane-mixed lastrow / lastcol states reading the last tile row / column"""
  return (32, 4, 125, 'perstate', dof == 2)


def expected_variant(lpt, c, n, cov, vel):
  """the static-covariance kernel variant (dgp_step_kernel_variant) a configuration must launch: 3 / 4 Woodbury (Q_c_inv = I, four states per
  lane, no velocity limits; exact fit / ragged), 1 block elimination (QK_STATIC), 0 general (non-diagonal Q_c_inv); None: per-call tensors, or the
  loop kernels of gn_long.h (n > 256)"""
  if n > 256: return None
  if cov == 'static_full': return 0
  if cov not in ('static', 'static_diag'): return None
  if cov == 'static' and c == 4 and not vel: return 3 if n == lpt * c else 4
  return 1


def oracle_qc(bt):
  """qc as the oracles take it: the dense blocks s_k Q_c_inv in 'scalar' modes"""
  return bt.qc_dense if is_scalar(bt.cov) else bt.qc


def okw(bt):
  """the C oracle's covariance arguments"""
  sh = (bt.B, bt.n, 1, 1)
  return dict(qc=oracle_qc(bt), ow=None if bt.ow is None else bt.ow.reshape(sh), eps=None if bt.eps is None else bt.eps.reshape(sh), q_full=bt.q_full)


def kkw(bt, io):
  """harness.Backend's covariance arguments"""
  return dict(qc=bt.qc, ow=bt.ow, eps=bt.eps, q_full=bt.q_full, io=io)


def raw_kw(bt, io):
  """harness.Backend's arguments of a 'scalar_raw' batch as the raw output vector (dgp_square_covariances in front of the kernels)"""
  return dict(raw=(bt.raw_out, bt.n - 1, True), io=io)


def rotate(bt, r):
  """the same batch with every per-trajectory input rolled by r trajectories (trajectory b goes to (b + r) % B)"""
  out = Batch()
  out.__dict__.update(bt.__dict__)
  roll = lambda a: a if a is None or a.shape[0] != bt.B else np.roll(a, r, axis=0)      # (a shared grid stays)
  for k in ('th', 'th_clean', 'start', 'goal', 'qc', 'ow', 'eps', 'qc_dense', 'raw_out', 'sdf'): setattr(out, k, roll(getattr(bt, k)))
  out.nan_rows = (bt.nan_rows + r) % bt.B
  return out


def ok_rows(bt):
  m = np.ones(bt.B, bool); m[bt.nan_rows] = False
  return m


# ---- checks: each returns a list of failure strings (empty: passed) ------------------------------------------------------------------
def _where(bt, b):
  w, l = locate(int(b), bt.lpt)
  return 'trajectory %d (wavefront %d, lane offset %d)' % (b, w, l)


def per_traj_rel(a, b):
  B = b.shape[0]
  num = np.abs(np.asarray(a, np.float64) - b).reshape(B, -1).max(1)
  den = np.maximum(np.abs(b).reshape(B, -1).max(1), 1e-300)
  r = num / den
  r[~np.isfinite(np.asarray(a, np.float64).reshape(B, -1)).all(1)] = np.inf
  return r


def check_close(bt, what, got, want, tol, rows=None, scale=None, limit=4):
  """per trajectory: max|got - want| / max|scale or want| < tol on `rows` (default: every non-NaN trajectory)"""
  rows = ok_rows(bt) if rows is None else rows
  if scale is None: e = per_traj_rel(got, want)
  else:
    B = want.shape[0]
    e = np.abs(np.asarray(got, np.float64) - want).reshape(B, -1).max(1) / np.maximum(np.abs(scale).reshape(B, -1).max(1), 1e-300)
    e[~np.isfinite(np.asarray(got, np.float64).reshape(B, -1)).all(1)] = np.inf
  bad = np.nonzero(rows & ~(e < tol))[0]
  return ['%s %s: %s rel err %.3g >= %.1g' % (bt.tag, what, _where(bt, b), e[b], tol) for b in bad[np.argsort(-e[bad])][:limit]] + \
         (['%s %s: ... %d trajectories in all' % (bt.tag, what, len(bad))] if len(bad) > limit else [])


def check_bit_equal(bt, what, a, a_rot, r, limit=4):
  """a: outputs of the batch, a_rot: of rotate(bt, r) -- every trajectory's outputs bit for bit (NaN == NaN)"""
  a = np.asarray(a); want = np.roll(a, r, axis=0)
  a_rot = np.asarray(a_rot)
  B = a.shape[0]
  same = ((a_rot == want) | (np.isnan(a_rot) & np.isnan(want)) if a.dtype.kind == 'f' else a_rot == want).reshape(B, -1).all(1)
  bad = np.nonzero(~same)[0]
  return ['%s %s not bit-equal under rotation by %d: %s' % (bt.tag, what, r, _where(bt, (b - r) % B)) for b in bad[:limit]] + \
         (['%s %s: ... %d trajectories in all' % (bt.tag, what, len(bad))] if len(bad) > limit else [])


def check_nan_isolation(bt, what, a_nan, a_clean):
  """the wave neighbours of every NaN trajectory: bit-equal to the same batch run without the NaN"""
  out = []
  T = tpw(bt.lpt)
  for b in bt.nan_rows:
    w = b // T
    for nb in range(w * T, min(bt.B, w * T + T)):
      if nb == b: continue
      if not np.array_equal(np.asarray(a_nan[nb]), np.asarray(a_clean[nb])):
        out.append('%s %s: NaN of trajectory %d reached its wave neighbour %s' % (bt.tag, what, b, _where(bt, nb)))
  return out


# ---- the directional-derivative check (e) ---------------------------------------------------------------------------------------------
FD_H = 1e-6        # central-difference step along v (v of unit size in th / start / goal / eps, relative size in qc / ow)


def direction(bt, seed=1):
  """a random direction over every per-trajectory differentiable input present (th, start, goal and, in per-state modes, qc, ow, eps)"""
  rs = np.random.RandomState(seed)
  v = dict(th=rs.uniform(-1, 1, bt.th.shape), start=rs.uniform(-1, 1, bt.start.shape), goal=rs.uniform(-1, 1, bt.goal.shape))
  if bt.qc is not None and bt.qc.ndim == 2:      # 'scalar': along delta s_k Q_c_inv (the backward returns the gradient of the blocks)
    v['qc'] = (rs.uniform(-1, 1, bt.qc.shape) * 0.1)[:, :, None, None] * bt.p.Q_c_inv
  elif bt.qc is not None:
    a = rs.uniform(-1, 1, bt.qc.shape) * 0.1
    v['qc'] = a + np.swapaxes(a, -1, -2)
  if bt.ow is not None: v['ow'] = rs.uniform(-1, 1, bt.ow.shape) * 100.0
  if bt.eps is not None: v['eps'] = rs.uniform(-1, 1, bt.eps.shape) * 0.1
  return v


def probe_lane(bt, b):
  """the lane whose rows the lane-resolved directional check probes in trajectory b: every lane of the trajectory, over the batch"""
  L = -(-bt.n // bt.c)
  return (b + b // tpw(bt.lpt)) % L


def lane_direction_qc(bt, g_qc, seed=3):
  """'scalar' modes: per trajectory, a direction over the GP blocks of the probed lane's factors (k = j C ... j C + C - 1) along delta s_k Q_c_inv,
  signed like <g_qc[k], Q_c_inv> -- a relative error e in that lane's block gradients moves the lane-resolved check by e"""
  rs = np.random.RandomState(seed)
  v = np.zeros(bt.qc.shape)
  for b in range(bt.B):
    j = probe_lane(bt, b)
    rows = slice(j * bt.c, min(bt.n - 1, (j + 1) * bt.c))
    v[b, rows] = np.sign(np.nan_to_num((g_qc[b, rows] * bt.p.Q_c_inv).sum((-1, -2)))) * rs.uniform(0.5, 1.0, v[b, rows].shape)
  return dict(qc=v[:, :, None, None] * bt.p.Q_c_inv)


def lane_direction(bt, g_th, seed=2):
  """per trajectory, a direction over the th rows of ONE lane (probe_lane; lane j holds states j C ... j C + C - 1), signed like the gradient
  under test so that the lane's terms add up: a relative error e in those rows moves <g, v> by e of sum |g v|, whatever n is"""
  rs = np.random.RandomState(seed)
  v = np.zeros(bt.th.shape)
  for b in range(bt.B):
    j = probe_lane(bt, b)
    rows = slice(j * bt.c, min(bt.n, (j + 1) * bt.c))
    v[b, rows] = np.sign(np.nan_to_num(g_th[b, rows])) * rs.uniform(0.5, 1.0, v[b, rows].shape)
  return dict(th=v)


def _loss(bt, x, gbar, gext, nthreads):
  from oracle import blocktri as BT
  sh = (bt.B, bt.n, 1, 1)
  d, _, ex, _ = BT.gn_step(bt.p, x['th'], x['start'], x['goal'], bt.sdf, qc=x.get('qc'), ow=None if x.get('ow') is None else x['ow'].reshape(sh),
                           eps=None if x.get('eps') is None else x['eps'].reshape(sh), q_full=bt.q_full, nthreads=nthreads, extended=True)
  return (gbar * d).reshape(bt.B, -1).sum(1) + gext * ex


def _decisions(bt, x):
  """everything piecewise about one step: the bilinear cell and hinge decision of every state, the velocity-limit decisions"""
  res = (bt.p.x_lims[1] - bt.p.x_lims[0]) / bt.sdf.shape[-1]
  px = np.floor(-bt.p.x_lims[0] / res + x['th'][:, :, 0] / res); py = np.floor(-bt.p.y_lims[0] / res - x['th'][:, :, 1] / res)
  out = [px, py, hinge_active(bt.p, bt.sdf, x['th'], x.get('eps'))]
  if bt.p.use_vel_limits: out.append((np.abs(x['th'][:, :, bt.dof:bt.dof + 2]) >= 1.0).reshape(bt.B, -1))
  return out


def directional(bt, grads, gbar, gext, v, nthreads=16, h=FD_H, loss=None):
  """-> (err (B,), excluded (B,) bool): |<g_b, v_b> - central difference of the extended-precision C oracle| / sum_i |g_i v_i|, per trajectory.
  Trajectories whose cell / hinge / velocity-limit decisions change within +-h v are excluded (the step is not differentiable there).
  loss: another function of the inputs (dict) -> (B,) to differentiate (default: the step's, <gbar, dtheta> + gext err_ext)."""
  x0 = dict(th=bt.th, start=bt.start, goal=bt.goal, qc=oracle_qc(bt), ow=bt.ow, eps=bt.eps)
  xp = {k: (None if a is None else a + h * v[k] if k in v else a) for k, a in x0.items()}
  xm = {k: (None if a is None else a - h * v[k] if k in v else a) for k, a in x0.items()}
  f = (lambda x: _loss(bt, x, gbar, gext, nthreads)) if loss is None else loss
  fd = (f(xp) - f(xm)) / (2 * h)
  terms = [(grads[k] * v[k]).reshape(bt.B, -1) for k in v]
  an = sum(t.sum(1) for t in terms)
  scale = np.maximum(sum(np.abs(t).sum(1) for t in terms), 1e-300)
  excl = np.zeros(bt.B, bool)
  d0, dp, dm = _decisions(bt, x0), _decisions(bt, xp), _decisions(bt, xm)
  for a, b_, c_ in zip(d0, dp, dm): excl |= ((a != b_) | (a != c_)).reshape(bt.B, -1).any(1)
  excl |= ~ok_rows(bt)
  err = np.abs(fd - an) / scale
  err[~np.isfinite(an)] = np.inf
  return err, excl


# ---- one configuration end to end ------------------------------------------------------------------------------------------------------
# the bounds of the directional checks (f64 kernels, h = 1e-6, 80-bit oracle).  FD_TOL, a direction over every input of the whole trajectory:
# measured on the MI355X over every trajectory of every configuration, 3.1e-7 at worst (q_full; 1e-9 ... 1e-8 typical).  Normalised by the whole
# trajectory's sum |g v|, it resolves gross errors only: one lane's share of that sum shrinks as n grows.  FD_LANE_TOL, a direction over the th rows
# of one lane per trajectory (lane_direction): a relative error e in that lane's rows moves it by e, so a 1e-3 error is flagged in any shape
# (tests/test_lane_mix.py::test_planted_gradient_lane_error, LPT = 64 and n = 256 included).
FD_TOL = 2e-6
FD_LANE_TOL = 1e-4      # (measured on the MI355X: 9e-7 at worst; 7e-8 on the CPU with the autograd oracle's gradients)
# the step of the lane-resolved check over g_qc ('scalar' modes): one lane's GP blocks move <gbar, dtheta> little (trajectories near their prior's optimum),
# and at FD_H the fp64 rounding of the oracle's dtheta alone gives up to 2.3e-4 of sum|g v| with the autograd oracle's exact gradients (160 trajectories,
# shape (16,1)); at 1e-4 -- rounding / h and truncation h^2 balanced -- 2e-6 at worst on the same trajectories
FD_H_QC = 1e-4
SDF_ROT_TOL = 7e-11      # the shared grid's gradient under rotation, of max|g_th|: see run_config


# ---- references of the errors kernels and of the twin families (B of run_config) ---------------------------------------------------------------
TWIN_STEP_TOL = {'f64': 1e-12, 'f32': 2e-6}      # dgp_gn_step_errors' dtheta / err / err_ext against dgp_gn_step on the same batch (parity_cases.case_step_errors)
UNW_TOL = {'f64': 1e-11, 'f32': 3e-5}            # the unweighted errors against oracle.gpmp2_oracle.unweighted_errors_batch (case_step_errors' tolv)
ERRS_BWD_TOL = 1e-7                              # f64 dgp_gn_step_errors_backward against its two halves run by hand (test_hip_every_step_errors_kernel)
SIBLING_TOL, SIBLING_SG_TOL = 1e-6, 2e-3         # fp32 against the fp64 sibling; g_start / g_goal of the errors' backward carry the start / goal error taken at
                                                 # th + dtheta summed in the I/O type (test_hip_every_f32_kernel_matches_its_f64_sibling)
TILED_STEP_TOL = {'f64': 1e-9, 'f32': 2e-4}      # tiled twins against the row-major kernels on the same batch (test_hip_every_tiled_twin_kernel)
TILED_GRAD_TOL = {'f64': 1e-7, 'f32': 2e-5}      # ... their gradients ('tight')
# f64 dgp_gn_solve_backward against the chain of single-step backward launches, per trajectory.  static_full: the general kernels' PCR rounds use explicit
# block inverses; per trajectory on the MI355X 6.2e-9 ... 7.1e-9 on 6 of 4096 trajectories of <3,64,4> (n = 253) and 6.9e-9 on one of <3,64,2> (n = 128), the
# rest below 5e-9 -- rounding, not a fault (a miscompiled kernel is off by 1e-3 and more): 3 x the worst measured
CHAIN_TOL = {'static': 1e-9, 'static_diag': 1e-9, 'static_full': 2e-8}
NEAR_H = 1e-9                                    # a state this close to a cell line, grid edge or hinge threshold: the kernel and the oracle may decide apart
EXCL_CAP = 0.005                                 # at most this share of the trajectories excluded by NEAR_H (and by the sibling's decisions)


def unweighted(bt, th, start=None, goal=None, eps=None):
  """oracle.gpmp2_oracle.unweighted_errors_batch -> (sg, gp, obs), each (B,) (the batch's start, goal, eps where not given)"""
  start = bt.start if start is None else start
  goal = bt.goal if goal is None else goal
  eps = bt.eps if eps is None else eps
  e = np.full((bt.B, bt.n, 1, 1), bt.p.epsilon_dist) if eps is None else np.reshape(eps, (bt.B, bt.n, 1, 1))
  with np.errstate(invalid='ignore'):      # (the NaN trajectories)
    sg, gp, ob = O.unweighted_errors_batch(th, start, goal, np.broadcast_to(bt.sdf, (bt.B,) + bt.sdf.shape[1:]), e, bt.p)
  return sg.reshape(-1), gp.reshape(-1), ob.reshape(-1)


def near_decision(bt, th, h=NEAR_H):
  """(B,) bool: a state of th within h of a bilinear cell line (the grid's edges included) or of its hinge threshold"""
  res = (bt.p.x_lims[1] - bt.p.x_lims[0]) / bt.sdf.shape[-1]
  px = -bt.p.x_lims[0] / res + th[:, :, 0] / res; py = -bt.p.y_lims[0] / res - th[:, :, 1] / res
  near = (np.abs(px - np.round(px)) * res < h) | (np.abs(py - np.round(py)) * res < h)
  e = bt.p.epsilon_dist if bt.eps is None else bt.eps.reshape(bt.B, bt.n)
  with np.errstate(invalid='ignore'):
    near |= np.abs(lookup(bt.p, bt.sdf, th[:, :, :2]) - (e + bt.p.radius)) < h
  return near.any(1)


def unw_autograd(bt, idx, cs, cg, co):
  """torch autograd of sum cs sg + cg gp + co obs (oracle/autograd_torch.unweighted_errors) on the trajectories idx -> dict th, start, goal, eps"""
  import torch
  from oracle import autograd_torch as AT
  m = len(idx)
  T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float64), requires_grad=True)
  x = dict(th=T(bt.th[idx]), start=T(bt.start[idx]), goal=T(bt.goal[idx]),
           eps=T(np.full((m, bt.n, 1, 1), bt.p.epsilon_dist) if bt.eps is None else bt.eps[idx].reshape(m, bt.n, 1, 1)))
  sdf = torch.tensor(np.ascontiguousarray(np.broadcast_to(bt.sdf, (bt.B,) + bt.sdf.shape[1:])[idx], np.float64))
  sg, gp, ob = AT.unweighted_errors(x['th'], x['start'], x['goal'], sdf, x['eps'], bt.p)
  c = lambda a: torch.tensor(np.asarray(a, np.float64)[idx])
  loss = (c(cs) * sg.reshape(-1)).sum() + (c(cg) * gp.reshape(-1)).sum() + (c(co) * ob.reshape(-1)).sum()
  keys = list(x)
  gr = torch.autograd.grad(loss, [x[k] for k in keys], allow_unused=True)
  return {k: (np.zeros(tuple(x[k].shape)) if g_ is None else g_.numpy()) for k, g_ in zip(keys, gr)}


def sibling_scale(ref, ok):
  """per-trajectory scale of a gradient check: max|ref_b|, floored at 1e-3 of the batch's largest entry (a trajectory whose gradient is all but zero)"""
  B = ref.shape[0]
  sc = np.maximum(np.abs(ref).reshape(B, -1).max(1), 1e-3 * np.abs(np.nan_to_num(ref[ok])).max())[:, None]
  return np.broadcast_to(sc, (B, ref[0].size))


def check_grads(bt, what, got, want, tol, ok, keys=('th', 'start', 'goal', 'qc', 'ow', 'eps'), tols=None):
  """check_close over the gradient tensors present in both dicts, on sibling_scale"""
  out = []
  for key in keys:
    if got.get(key) is None or want.get(key) is None: continue
    w = np.asarray(want[key], np.float64)
    out += check_close(bt, '%s g_%s' % (what, key), np.asarray(got[key]).reshape(bt.B, -1), w.reshape(bt.B, -1), (tols or {}).get(key, tol), rows=ok,
                       scale=sibling_scale(w, ok))
  return out


def chain_walk(be, bt, K, hist, tho, its, gbar, io, gm):
  """the gradients of dgp_gn_solve_backward by hand: single-step backward launches walked back through the traced history -> dict th, start, goal"""
  gcur = np.asarray(gbar, np.float64).copy()
  acc = dict(start=np.zeros(bt.start.shape), goal=np.zeros(bt.goal.shape))
  for k in range(K - 1, -1, -1):
    on = (its > k)[:, None, None]
    thk = np.where(on, np.nan_to_num(hist[k]), tho)
    nxt = np.where((its > k + 1)[:, None, None], np.nan_to_num(hist[min(k + 1, K - 1)]), tho)
    one = be.backward(bt.p, thk, bt.start, bt.goal, bt.sdf, nxt - thk, gcur * on, None, io=io, sdf_grad=gm)
    gcur = gcur + one['th'] * on
    acc['start'] += one['start'] * on; acc['goal'] += one['goal'] * on
  return dict(th=gcur, **acc)


def raw_expect(bt, g):
  """d/d out of 'scalar_raw' by hand from the gradients of the squared tensors: 2 out trace(g_qc) (Q_c_inv = I), 2 out g_ow, 2 out g_eps"""
  n, o = bt.n, bt.raw_out
  return np.concatenate([2.0 * o[:, :n - 1] * np.einsum('bkii->bk', g['qc']), 2.0 * o[:, n - 1:2 * n - 1] * g['ow'], 2.0 * o[:, 2 * n - 1:] * g['eps']], 1)


def stopping(bt, okw_, tol, K, nthreads, band, io_round=False):
  """K chained C-oracle steps under the fused loop's stopping rule (stop after the step whose norm is < tol) -> th_out, iters, near (B,) bool:
  a step norm within `band` (relative) of tol -- the kernel may legitimately stop one iteration apart"""
  from oracle import blocktri as BT
  cur = bt.th.copy(); its = np.zeros(bt.B, np.int32); on = np.ones(bt.B, bool); near = np.zeros(bt.B, bool)
  for k in range(K):
    d, _, _, _ = BT.gn_step(bt.p, cur, bt.start, bt.goal, bt.sdf, nthreads=nthreads, **okw_)
    nrm = np.sqrt((d.reshape(bt.B, -1) ** 2).sum(1))
    near |= on & (np.abs(nrm - tol) <= band * tol)
    cur[on] += d[on]; its[on] = k + 1
    if io_round: cur = PC.rnd(cur, 'f32')
    on &= ~(nrm < tol)
  return cur, its, near


def autograd_picks(bt):
  """the trajectories of the sampled autograd check: the first wavefront (its mixed slot 0 and its last slot), a middle wavefront without a NaN
  (mixed slot 0 and a slot at another lane offset; the next wavefront as well for LPT = 64) and the ragged last wavefront -- at least 4, one mixed"""
  T = tpw(bt.lpt)
  W = bt.waves + (T > 1)
  mid = bt.waves // 2
  while mid in set((bt.nan_rows // T).tolist()): mid += 1
  picks = [0, T - 1, mid * T, mid * T + T // 2, (mid + 1) * T, bt.B - 1] if T > 1 else [0, 1, mid, mid + 1, bt.B - 1]
  picks = sorted(set(b for b in picks if 0 <= b < bt.B) - set(bt.nan_rows.tolist()))
  assert len(picks) >= 4 and picks[-1] // T == W - 1
  return picks


def median_tol(dth):
  """tol_delta of the K = 3 loop checks: the median first-step norm -- taken halfway between the two middle norms, so that no trajectory's
  norm equals it"""
  nrm = np.sort(np.sqrt((dth.reshape(dth.shape[0], -1) ** 2).sum(1)))
  m = len(nrm) // 2
  return float(0.5 * (nrm[max(m - 1, 0)] + nrm[m]))


def run_config(be, bt, nthreads=16, fd=True, autograd=True, extra=True, report=None, long=False):
  """Parts (a)-(f) of tests/test_hip_full_batch.py on one lane-mixed batch (fp32-exact numbers), fp64 and fp32 I/O kernels -> list of failures.
  report: a dict that receives the counts (wavefronts, excluded trajectories of (b) and (e), worst errors)."""
  from oracle import blocktri as BT
  from dgpmp2_amd import _capi
  import harness
  bad = []
  rep = {} if report is None else report
  rep.update(waves=bt.waves + (tpw(bt.lpt) > 1), B=bt.B)
  ok = ok_rows(bt)
  scal = is_scalar(bt.cov)      # (DGP_QC_SCALAR: a step-only mode -- no fused loop, no traced loop)
  want_v = expected_variant(bt.lpt, bt.c, bt.n, bt.cov, bt.p.use_vel_limits)
  if want_v is not None:      # the static kernel variant this batch launches under the forced shape: no silent fall-back to another family
    rep['variant'] = (_capi.Solver(harness.config_from_oracle(bt.p, 'f64'), api=be.api).step_kernel_variant(bt.B), bt.c)
    if rep['variant'][0] != want_v: bad.append('%s: static kernel variant %d, expected %d' % (bt.tag, rep['variant'][0], want_v))
  cs, cg, co = (PC.rnd(np.random.RandomState(8 + i).randn(bt.B), 'f32') for i in range(3))      # cotangents of unw_sg, unw_gp, unw_obs
  K = 3
  r = tpw(bt.lpt) // 2 + 1
  rbt = rotate(bt, r)
  rs = np.random.RandomState(7)
  gbar = PC.rnd(rs.randn(bt.B, bt.n, 2 * bt.dof), 'f32'); gext = PC.rnd(rs.randn(bt.B), 'f32')
  c_dth, c_err, c_eex, _ = BT.gn_step(bt.p, bt.th, bt.start, bt.goal, bt.sdf, nthreads=nthreads, **okw(bt))
  tol = median_tol(c_dth[ok])
  rep['tol_delta'] = tol
  out = {}
  for io in ('f64', 'f32'):
    kw = kkw(bt, io)
    rkw = kkw(rbt, io)
    gm = 'f64' if io == 'f32' and not long else 'dense'      # (long trajectories: no float64 partial grids for fp32 I/O)
    t = '[%s] ' % io
    o = out[io] = {}
    # (a) one step against the C oracle
    dth, err, eex, info = o['step'] = be.step(bt.p, bt.th, bt.start, bt.goal, bt.sdf, **kw)
    wide = 10 if bt.n > 512 else 1      # (cond(Lambda) grows with n: the fp64 oracles themselves differ by that much, parity_cases.case_long_trajectories)
    bad += check_close(bt, t + 'step dtheta', dth, c_dth, wide * PC.TOL[io])
    bad += check_close(bt, t + 'step err', err[:, None], c_err[:, None], 10 * PC.TOL_ERR[io])
    bad += check_close(bt, t + 'step err_ext', eex[:, None], c_eex[:, None], 10 * PC.TOL_ERR[io])
    rep['err_worst_' + io] = float(max(np.max(per_traj_rel(err[ok, None], c_err[ok, None])), np.max(per_traj_rel(eex[ok, None], c_eex[ok, None]))))
    bad += ['%s %s step info %d: %s' % (bt.tag, t, info[b], _where(bt, b)) for b in np.nonzero(ok & (info != 0))[0][:4]]
    # dgp_eval_errors at th (MODE_EVAL): err / err_ext against the C oracle, the unweighted errors against unweighted_errors_batch
    ekw, rekw = (dict(kw, qc=bt.qc_dense), dict(rkw, qc=rbt.qc_dense)) if scal else (kw, rkw)      # (dgp_eval_errors takes the dense blocks)
    ev = o['eval'] = be.eval_errors(bt.p, bt.th, bt.start, bt.goal, bt.sdf, **ekw)
    bad += check_close(bt, t + 'eval_errors err', ev[0][:, None], c_err[:, None], 10 * PC.TOL_ERR[io])
    bad += check_close(bt, t + 'eval_errors err_ext', ev[1][:, None], c_eex[:, None], 10 * PC.TOL_ERR[io])
    if 'unw_th' not in out: out['unw_th'] = (unweighted(bt, bt.th), near_decision(bt, bt.th))
    u_ref, near0 = out['unw_th']
    rep['eval_excluded'] = int((near0 & ok).sum())
    if (near0 & ok).sum() > EXCL_CAP * ok.sum(): bad.append('%s %s eval_errors: %d of %d trajectories within %g of a decision' % (bt.tag, t, (near0 & ok).sum(), ok.sum(), NEAR_H))
    for i, name in enumerate(('unw_sg', 'unw_gp', 'unw_obs')):
      bad += check_close(bt, t + 'eval_errors ' + name, ev[2 + i][:, None], u_ref[i][:, None], UNW_TOL[io], rows=ok & ~near0)
    rep['eval_unw_worst_' + io] = float(max(np.max(per_traj_rel(ev[2 + i][ok & ~near0, None], u_ref[i][ok & ~near0, None]), initial=0.0) for i in range(3)))
    if scal:      # the fused loop refuses DGP_QC_SCALAR
      try:
        be.solve(bt.p, bt.th, bt.start, bt.goal, bt.sdf, K, tol, **kw)
        bad.append('%s %s dgp_gn_solve accepted DGP_QC_SCALAR' % (bt.tag, t))
      except _capi.DgpError as ex:
        if ex.code != _capi.DGP_EUNSUPPORTED: bad.append('%s %s dgp_gn_solve with DGP_QC_SCALAR: %s' % (bt.tag, t, ex))
    # (b) the fused loop, iteration counts mixed inside the wavefronts
    if not scal:
      tho, its, eh, eeh, ef, sinfo = o['solve'] = be.solve(bt.p, bt.th, bt.start, bt.goal, bt.sdf, K, tol, **kw)
      # (the loop kernels of gn_long.h keep the state in th_out, of the I/O type: for fp32 I/O the oracle chain rounds the trajectory to fp32 as well)
      key = 'chain_f32' if long and io == 'f32' else 'chain'
      if key not in out: out[key] = stopping(bt, okw(bt), tol, K, nthreads, 1e-6, io_round=key == 'chain_f32')
      c_tho, c_its, near = out[key]
      rep['b_excluded'] = int((near & ok).sum())
      if (near & ok).sum() > 0.005 * ok.sum(): bad.append('%s %s fused loop: %d of %d trajectories stop within rounding of tol_delta' % (bt.tag, t, (near & ok).sum(), ok.sum()))
      keep = ok & ~near
      bad += check_close(bt, t + 'fused loop th_out', tho, c_tho, wide * (1e-7 if io == 'f64' else 1e-5), rows=keep)
      bad += ['%s %s fused loop iters %d, oracle %d: %s' % (bt.tag, t, its[b], c_its[b], _where(bt, b)) for b in np.nonzero(keep & (its != c_its))[0][:4]]
      bad += ['%s %s fused loop info %d: %s' % (bt.tag, t, sinfo[b], _where(bt, b)) for b in np.nonzero(ok & (sinfo != 0))[0][:4]]
    # the backward with the step's own dtheta
    g = o['backward'] = be.backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, dth, gbar, gext, sdf_grad=gm, **kw)
    # (c) batch-position independence: the same batch rotated
    rstep = be.step(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, **rkw)
    for name, a, b_ in zip(('dtheta', 'err', 'err_ext', 'info'), o['step'], rstep): bad += check_bit_equal(bt, t + 'step ' + name, a, b_, r)
    if not scal:
      rsol = be.solve(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, K, tol, **rkw)
      for name, a, b_ in zip(('th_out', 'iters', 'err_hist', 'errext_hist', 'err_final', 'info'), o['solve'], rsol): bad += check_bit_equal(bt, t + 'fused loop ' + name, a, b_, r)
    rg = be.backward(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, np.roll(dth, r, 0), np.roll(gbar, r, 0), np.roll(gext, r, 0), sdf_grad=gm, **rkw)
    for key in ('th', 'start', 'goal', 'qc', 'ow', 'eps'):
      if g[key] is not None: bad += check_bit_equal(bt, t + 'backward g_' + key, g[key], rg[key], r)
    rev = be.eval_errors(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, **rekw)
    for name, a, b_ in zip(('err', 'err_ext', 'unw_sg', 'unw_gp', 'unw_obs'), o['eval'], rev): bad += check_bit_equal(bt, t + 'eval_errors ' + name, a, b_, r)
    raw_tol = 1e-13 if io == 'f64' else 3e-6      # (parity_cases.case_raw_squared_covariances)
    if bt.raw_out is not None:      # the same squares as the learn module's raw output vector: dgp_square_covariances (+ _backward) at full batch
      sa = be.step(bt.p, bt.th, bt.start, bt.goal, bt.sdf, **raw_kw(bt, io))
      for name, a, b_ in zip(('dtheta', 'err', 'err_ext', 'info'), o['step'], sa): bad += check_bit_equal(bt, t + 'raw step ' + name, a, b_, 0)
      ga_ = be.backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, dth, gbar, gext, sdf_grad=gm, **raw_kw(bt, io))
      for key in ('th', 'start', 'goal'): bad += check_bit_equal(bt, t + 'raw backward g_' + key, g[key], ga_[key], 0)
      bad += check_close(bt, t + 'raw backward d/d out', ga_['out'], raw_expect(bt, g), raw_tol, rows=ok)
      gr_ = be.backward(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, np.roll(dth, r, 0), np.roll(gbar, r, 0), np.roll(gext, r, 0), sdf_grad=gm, **raw_kw(rbt, io))
      bad += check_bit_equal(bt, t + 'raw backward d/d out', ga_['out'], gr_['out'], r)
    if extra:
      fam = []
      if bt.cov in ('static', 'static_diag', 'static_full'): fam.append('traced')
      if bt.c == 4 and bt.lpt <= 32: fam += ['step_errors', 'tiled']
      for f in fam:
        if f == 'traced':
          a = be.solve_traced(bt.p, bt.th, bt.start, bt.goal, bt.sdf, K, tol, io=io)
          if not (np.array_equal(a[0], tho, equal_nan=True) and np.array_equal(a[1], its)): bad.append('%s %s traced loop differs from the plain loop' % (bt.tag, t))
          b_ = be.solve_traced(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, K, tol, io=io)
          for name, x, y in (('th_out', a[0], b_[0]), ('iters', a[1], b_[1]), ('th_hist', np.swapaxes(a[2], 0, 1), np.swapaxes(b_[2], 0, 1))): bad += check_bit_equal(bt, t + 'traced loop ' + name, x, y, r)
          hist = a[2]
          ca = be.solve_backward(bt.p, bt.start, bt.goal, bt.sdf, K, hist, a[0], a[1], gbar, io=io, sdf_grad=gm)
          cb = be.solve_backward(rbt.p, rbt.start, rbt.goal, rbt.sdf, K, np.roll(hist, r, 1), b_[0], b_[1], np.roll(gbar, r, 0), io=io, sdf_grad=gm)
          for key in ('th', 'start', 'goal'): bad += check_bit_equal(bt, t + 'chain backward g_' + key, ca[key], cb[key], r)
          # the chain backward against the single-step backward launches walked by hand through the history (f64), fp32 against its fp64 sibling
          if io == 'f64':
            cw = chain_walk(be, bt, K, hist, a[0], a[1], gbar, io, gm)
            bad += check_grads(bt, t + 'chain backward vs chained steps', ca, cw, CHAIN_TOL[bt.cov], ok, keys=('th', 'start', 'goal'))
            rep['chain_worst'] = float(max(np.max(per_traj_rel(ca[k][ok], cw[k][ok]), initial=0.0) for k in ('th', 'start', 'goal')))
          else:
            c64 = be.solve_backward(bt.p, bt.start, bt.goal, bt.sdf, K, hist, a[0], a[1], gbar, io='f64', sdf_grad='dense')
            bad += check_grads(bt, t + 'chain backward vs f64 sibling', ca, c64, SIBLING_TOL, ok, keys=('th', 'start', 'goal'))
        if f == 'step_errors':
          a = be.step_errors(bt.p, bt.th, bt.start, bt.goal, bt.sdf, **kw); b_ = be.step_errors(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, **rkw)
          for name, x, y in zip(('dtheta', 'err', 'err_ext', 'info', 'unw_sg', 'unw_gp', 'unw_obs'), a, b_): bad += check_bit_equal(bt, t + 'step_errors ' + name, x, y, r)
          # (1) dtheta / err / err_ext against the standard step of this batch (held to the C oracle in (a)); the unweighted errors at th + dtheta,
          #     summed in the I/O type from the kernel's own dtheta as the kernel sums it, against unweighted_errors_batch
          for i, name in enumerate(('dtheta', 'err', 'err_ext')):
            bad += check_close(bt, t + 'step_errors %s vs step' % name, a[i].reshape(bt.B, -1), o['step'][i].reshape(bt.B, -1), TWIN_STEP_TOL[io])
          npdt = np.float64 if io == 'f64' else np.float32
          thn = (bt.th.astype(npdt) + a[0].astype(npdt)).astype(np.float64)
          u_new, nearn = unweighted(bt, thn), near_decision(bt, thn)
          rep['errs_excluded_' + io] = int((nearn & ok).sum())
          if (nearn & ok).sum() > EXCL_CAP * ok.sum(): bad.append('%s %s step_errors: %d of %d trajectories within %g of a decision' % (bt.tag, t, (nearn & ok).sum(), ok.sum(), NEAR_H))
          for i, name in enumerate(('unw_sg', 'unw_gp', 'unw_obs')):
            bad += check_close(bt, t + 'step_errors ' + name, a[4 + i][:, None], u_new[i][:, None], UNW_TOL[io], rows=ok & ~nearn)
          rep['errs_unw_worst_' + io] = float(max(np.max(per_traj_rel(a[4 + i][ok & ~nearn, None], u_new[i][ok & ~nearn, None]), initial=0.0) for i in range(3)))
          x = be.step_errors_backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, a[0], gbar, gext, cs, cg, co, sdf_grad='none', **kw)
          y = be.step_errors_backward(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, b_[0], np.roll(gbar, r, 0), np.roll(gext, r, 0), np.roll(cs, r, 0), np.roll(cg, r, 0), np.roll(co, r, 0), sdf_grad='none', **rkw)
          for key in ('th', 'start', 'goal', 'qc', 'ow', 'eps'):
            if x[key] is not None: bad += check_bit_equal(bt, t + 'step_errors backward g_' + key, x[key], y[key], r)
          # (2) the backward against its two halves run by hand (f64: dgp_eval_errors_backward at th + dtheta, then dgp_gn_step_backward with the summed
          #     cotangent), fp32 against its fp64 sibling on the same numbers
          if io == 'f64':
            h1 = be.eval_backward(bt.p, thn, bt.start, bt.goal, bt.sdf, None, cs, cg, co, eps=bt.eps, io=io, want_sdf=False)
            h2 = be.backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, a[0], gbar + h1['th'], gext, sdf_grad=gm, **kw)
            want = dict(th=h2['th'] + h1['th'], start=h2['start'] + h1['start'], goal=h2['goal'] + h1['goal'], qc=h2['qc'], ow=h2['ow'],
                        eps=None if bt.eps is None else h2['eps'] + h1['eps'])
            bad += check_grads(bt, t + 'step_errors backward vs its halves', x, want, ERRS_BWD_TOL, ok)
            rep['errs_bwd_worst'] = float(max(np.max(per_traj_rel(x[k][ok], want[k][ok]), initial=0.0) for k in want if want[k] is not None))
          else:
            # (the fp64 sibling sums th + dtheta in fp64, up to 2.4e-7 away from the fp32 sum: a state of th + dtheta that close to a cell line or hinge
            #  threshold is decided apart by the two kernels -- 1.04e-7 from a cell line gave 2.7e-3 in g_eps, shape (16,4) scalar_raw -- such trajectories,
            #  whose cell / hinge decisions at the two sums differ, are excluded and counted)
            x64 = be.step_errors_backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, a[0], gbar, gext, cs, cg, co, sdf_grad='none', **kkw(bt, 'f64'))
            x_e = dict(th=thn, eps=bt.eps); x_e64 = dict(th=bt.th + a[0], eps=bt.eps)
            nears = np.zeros(bt.B, bool)
            with np.errstate(invalid='ignore'):
              for u, w in zip(_decisions(bt, x_e), _decisions(bt, x_e64)): nears |= (u != w).reshape(bt.B, -1).any(1)
            rep['errs_sibling_excluded'] = int((nears & ok).sum())
            if (nears & ok).sum() > EXCL_CAP * ok.sum(): bad.append('%s %s step_errors sibling: %d of %d trajectories decided apart at th + dtheta' % (bt.tag, t, (nears & ok).sum(), ok.sum()))
            bad += check_grads(bt, t + 'step_errors backward vs f64 sibling', x, x64, SIBLING_TOL, ok & ~nears, tols=dict(start=SIBLING_SG_TOL, goal=SIBLING_SG_TOL))
          if bt.raw_out is not None:
            ea = be.step_errors(bt.p, bt.th, bt.start, bt.goal, bt.sdf, **raw_kw(bt, io))
            for name, x_, y_ in zip(('dtheta', 'err', 'err_ext', 'info', 'unw_sg', 'unw_gp', 'unw_obs'), a, ea): bad += check_bit_equal(bt, t + 'raw step_errors ' + name, x_, y_, 0)
            fa = be.step_errors_backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, a[0], gbar, gext, cs, cg, co, sdf_grad='none', **raw_kw(bt, io))
            bad += check_close(bt, t + 'raw step_errors backward d/d out', fa['out'], raw_expect(bt, x), raw_tol, rows=ok)
        if f == 'tiled':
          bt_ = harness.Backend(be.kind); bt_.sdf_tiled = True
          a = bt_.step(bt.p, bt.th, bt.start, bt.goal, bt.sdf, **kw); b_ = bt_.step(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, **rkw)
          for name, x, y in zip(('dtheta', 'err', 'err_ext', 'info'), a, b_): bad += check_bit_equal(bt, t + '[tiled] step ' + name, x, y, r)
          x = bt_.backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, dth, gbar, gext, sdf_grad=gm, **kw)
          y = bt_.backward(rbt.p, rbt.th, rbt.start, rbt.goal, rbt.sdf, np.roll(dth, r, 0), np.roll(gbar, r, 0), np.roll(gext, r, 0), sdf_grad=gm, **rkw)
          for key in ('th', 'start', 'goal', 'qc', 'ow', 'eps'):
            if x[key] is not None: bad += check_bit_equal(bt, t + '[tiled] backward g_' + key, x[key], y[key], r)
          # (4) step and backward against the row-major kernels on the same batch (held to the oracles in (a) and (e))
          for i, name in enumerate(('dtheta', 'err', 'err_ext')):
            bad += check_close(bt, t + '[tiled] step %s vs row-major' % name, a[i].reshape(bt.B, -1), o['step'][i].reshape(bt.B, -1), TILED_STEP_TOL[io])
          bad += check_grads(bt, t + '[tiled] backward vs row-major', x, g, TILED_GRAD_TOL[io], ok)
          rep['tiled_worst_' + io] = float(max(np.max(per_traj_rel(x[k][ok], g[k][ok]), initial=0.0) for k in ('th', 'start', 'goal', 'qc', 'ow', 'eps') if g[k] is not None))
    # (f) NaN isolation: the NaN trajectories' wave neighbours against the same batch without the NaN
    if len(bt.nan_rows):
      cl = be.step(bt.p, bt.th_clean, bt.start, bt.goal, bt.sdf, **kw)
      for name, a, b_ in zip(('dtheta', 'err', 'err_ext', 'info'), o['step'], cl): bad += check_nan_isolation(bt, t + 'step ' + name, a, b_)
      gc = be.backward(bt.p, bt.th_clean, bt.start, bt.goal, bt.sdf, np.where(np.isnan(dth), 0.0, dth), gbar, gext, sdf_grad=gm, **kw)
      for key in ('th', 'start', 'goal'): bad += check_nan_isolation(bt, t + 'backward g_' + key, g[key], gc[key])
    # the shared grid's gradient (summed by atomics, in an order that may change): to 1e-12 of max|g_th| under rotation, on the batch without the NaN
    th_c, rth_c = (bt.th_clean, rbt.th_clean) if len(bt.nan_rows) else (bt.th, rbt.th)
    d_c = be.step(bt.p, th_c, bt.start, bt.goal, bt.sdf, **kw)[0]
    ga = be.backward(bt.p, th_c, bt.start, bt.goal, bt.sdf, d_c, gbar, gext, sdf_grad=gm, **kw)
    gb = be.backward(rbt.p, rth_c, rbt.start, rbt.goal, rbt.sdf, np.roll(d_c, r, 0), np.roll(gbar, r, 0), np.roll(gext, r, 0), sdf_grad=gm, **rkw)
    # (measured up to 6.8e-12 of max|g_th| on the MI355X, 2.6e-12 on the emulator at 14 trajectories: a cell of the grid gradient sums thousands of
    #  contributions whose float64 atomics land in another order -- 1e-12 of max|g_th| cannot hold; SDF_ROT_TOL is 10 x the measured worst)
    # (long trajectories, fp32 I/O: the grid gradient is summed by fp32 atomics in an order that changes from run to run -- left out)
    es = 0.0 if long and io == 'f32' else np.abs(gb['sdf'].sum(0) - ga['sdf'].sum(0)).max() / max(np.abs(ga['th']).max(), 1e-300)
    rep['sdf_rotation_' + io] = float(es)
    if not es <= SDF_ROT_TOL: bad.append('%s %s backward g_sdf (shared grid, atomics) under rotation: %.3g of max|g_th|' % (bt.tag, t, es))
  # (d) fp32 against the fp64 siblings on the full batch (the same numbers; the fp32 dtheta into both backward kernels)
  stol = 1e-6
  f32, f64 = out['f32']['step'], out['f64']['step']
  bad += check_close(bt, 'sibling step dtheta', f32[0], f64[0], stol)
  bad += check_close(bt, 'sibling step err', f32[1][:, None], f64[1][:, None], stol)
  bad += check_close(bt, 'sibling step err_ext', f32[2][:, None], f64[2][:, None], stol)
  d32 = out['f32']['step'][0]
  up = lambda a: None if a is None else np.asarray(a, np.float64)
  g64 = be.backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, d32, gbar, gext, sdf_grad='dense', **kkw(bt, 'f64'))
  for key in ('th', 'start', 'goal', 'qc', 'ow', 'eps'):
    if g64[key] is None: continue
    sc = np.maximum(np.abs(g64[key]).reshape(bt.B, -1).max(1), 1e-3 * np.abs(np.nan_to_num(g64[key][ok])).max())[:, None]
    bad += check_close(bt, 'sibling backward g_' + key, out['f32']['backward'][key].reshape(bt.B, -1), g64[key].reshape(bt.B, -1), stol, scale=np.broadcast_to(sc, (bt.B, g64[key][0].size)))
  s32, s64 = out['f32'].get('solve'), out['f64'].get('solve')
  same = ok & (s32[1] == s64[1]) if s32 is not None else None
  if not long and s32 is not None: bad += check_close(bt, 'sibling fused loop th_out', s32[0], s64[0], stol, rows=same & ~out['chain'][2])      # (long: the fp32 loop's state is fp32)
  # (e) backward against independent references (f64 kernels)
  g = out['f64']['backward']
  if autograd:
    from oracle import autograd_torch as AT
    T_ = tpw(bt.lpt)
    picks = autograd_picks(bt)
    idx = np.array(picks)
    sub = lambda a: None if a is None else a[idx]
    sdf_s = bt.sdf if bt.sdf.shape[0] == 1 else bt.sdf[idx]
    go = AT.step_gradients(bt.p, bt.th[idx], bt.start[idx], bt.goal[idx], sdf_s, gbar[idx], gext[idx], qc=sub(oracle_qc(bt)), ow=sub(bt.ow), eps=sub(bt.eps), q_full=bt.q_full)
    for key in ('th', 'start', 'goal', 'qc', 'ow', 'eps'):
      if g[key] is None: continue
      a, b_ = g[key][idx], go[key].reshape(g[key][idx].shape)
      e = np.abs(a - b_).reshape(len(idx), -1).max(1) / np.maximum(np.abs(b_).reshape(len(idx), -1).max(1), 1e-300)
      for i in np.nonzero(~(e < 1e-6))[0]: bad.append('%s autograd g_%s: %s rel err %.3g' % (bt.tag, key, _where(bt, idx[i]), e[i]))
    rep['autograd_samples'] = [locate(b, bt.lpt) for b in picks]
    if not (len(picks) >= 4 and any(bt.kinds[b] == 'mixed' for b in picks)): bad.append('%s autograd samples %s' % (bt.tag, rep['autograd_samples']))
  # (3) dgp_eval_errors_backward (f64) at th: against torch autograd of the unweighted errors on the sampled trajectories, and a central difference
  #     of unweighted_errors_batch along direction(bt) on every trajectory (the same exclusion rule as the step's)
  ge = be.eval_backward(bt.p, bt.th, bt.start, bt.goal, bt.sdf, None, cs, cg, co, eps=bt.eps, io='f64', want_sdf=False)
  if autograd:
    gu = unw_autograd(bt, idx, cs, cg, co)
    for key in ('th', 'start', 'goal', 'eps'):
      if ge[key] is None: continue
      a, b_ = ge[key][idx], gu[key].reshape(ge[key][idx].shape)
      e = np.abs(a - b_).reshape(len(idx), -1).max(1) / np.maximum(np.abs(b_).reshape(len(idx), -1).max(1), 1e-300)
      for i in np.nonzero(~(e < 1e-6))[0]: bad.append('%s eval_errors backward autograd g_%s: %s rel err %.3g' % (bt.tag, key, _where(bt, idx[i]), e[i]))
  if fd:
    vu = {k: a for k, a in direction(bt, seed=4).items() if k in ('th', 'start', 'goal', 'eps')}
    lossu = lambda x: sum(c_ * u for c_, u in zip((cs, cg, co), unweighted(bt, x['th'], x['start'], x['goal'], x['eps'])))
    err, excl = directional(bt, ge, None, None, vu, nthreads=nthreads, loss=lossu)
    rep['eval_fd_excluded'] = int(excl.sum() - (~ok).sum())
    rep['eval_fd_worst'] = float(np.max(err[~excl])) if (~excl).any() else 0.0
    bad += ['%s eval_errors backward directional derivative: %s |<g,v> - FD| / sum|g v| = %.3g >= %.1g' % (bt.tag, _where(bt, b), err[b], FD_TOL) for b in np.nonzero(~excl & ~(err < FD_TOL))[0][:4]]
  if fd:
    v = direction(bt)
    err, excl = directional(bt, g, gbar, gext, v, nthreads=nthreads)
    rep['e_excluded'] = int(excl.sum() - (~ok).sum())
    rep['fd_worst'] = float(np.max(err[~excl])) if (~excl).any() else 0.0
    bad += ['%s directional derivative: %s |<g,v> - FD| / sum|g v| = %.3g >= %.1g' % (bt.tag, _where(bt, b), err[b], FD_TOL) for b in np.nonzero(~excl & ~(err < FD_TOL))[0][:4]]
    err, excl = directional(bt, g, gbar, gext, lane_direction(bt, g['th']), nthreads=nthreads)
    rep['lane_excluded'] = int(excl.sum() - (~ok).sum())
    rep['fd_lane_worst'] = float(np.max(err[~excl])) if (~excl).any() else 0.0
    bad += ['%s lane directional derivative (lane %d): %s |<g,v> - FD| / sum|g v| = %.3g >= %.1g' % (bt.tag, probe_lane(bt, b), _where(bt, b), err[b], FD_LANE_TOL)
            for b in np.nonzero(~excl & ~(err < FD_LANE_TOL))[0][:4]]
    if scal:      # ... and over the GP blocks of one lane's factors: the scaled backward's g_qc lane by lane
      err, excl = directional(bt, g, gbar, gext, lane_direction_qc(bt, g['qc']), nthreads=nthreads, h=FD_H_QC)
      rep['fd_lane_qc_worst'] = float(np.max(err[~excl])) if (~excl).any() else 0.0
      bad += ['%s lane directional derivative over g_qc (lane %d): %s |<g,v> - FD| / sum|g v| = %.3g >= %.1g' % (bt.tag, probe_lane(bt, b), _where(bt, b), err[b], FD_LANE_TOL)
              for b in np.nonzero(~excl & ~(err < FD_LANE_TOL))[0][:4]]
  return bad


# ---- the headline configurations, 10 GN iterations at full size (BASELINE.json configs[1..3]) ------------------------------------------------
HEADLINE = {'configs[1]': (2, 256, {}), 'configs[2]': (2, 256, dict(use_vel_limits=True)), 'configs[3]': (3, 512, dict(non_holonomic=True))}
# final trajectory against 10 untethered C-oracle steps, of max|th_b|, hinge-grazing trajectories excluded: 10 x the worst measured on the MI355X
# (configs[1]: 2.4e-8 / 2.5e-7, configs[2]: 3.0e-7 / 2.9e-7 for fp64 / fp32 I/O).  configs[3] (d = 6, non-holonomic) is still far from converged
# after 10 iterations and amplifies rounding chaotically: 0.44 of |th| measured with no hinge change while the teacher-forced steps agree to 3e-11 --
# there the teacher forcing is the check and the untethered bound (10 x measured) only catches gross faults.
UNTETHERED_TOL = {('configs[1]', 'f64'): 2.5e-7, ('configs[1]', 'f32'): 2.5e-6, ('configs[2]', 'f64'): 3e-6, ('configs[2]', 'f32'): 3e-6,
                  ('configs[3]', 'f64'): 4.4, ('configs[3]', 'f32'): 4.4}
# 10 chained fp32 dgp_gn_step launches against the fused loop, of max|th_b|, trajectories whose hinge set differs excluded: the launches round the
# trajectory to fp32 between the steps and the loop does not, and a state that crosses a grid cell line moves J discontinuously -- measured 1.5e-2 at
# worst on the MI355X (41 of 4096 trajectories changed hinge set), so 10 x that; every one of the chained launches is held to the C oracle's step from
# the same fp32 trajectory at PC.TOL['f32'] besides.
CHAIN_F32_TOL = 0.15


def headline_batch(name, B=4096, n=64, seed=0):
  """the benchmark's inputs (bench.py make_inputs: straight lines between U(-4,4)^2 starts and goals, the three-circle grid; d = 6: headings 0 -> pi/2), fp32-exact"""
  dof, G_, kw = HEADLINE[name]
  rs = np.random.RandomState(seed)
  bt = Batch()
  bt.p = O.OracleParams(dof=dof, total_time_step=n - 1, **kw)
  d = 2 * dof
  start = np.zeros((B, 1, d)); goal = np.zeros((B, 1, d))
  start[:, 0, :2] = rs.uniform(-4, 4, (B, 2)); goal[:, 0, :2] = rs.uniform(-4, 4, (B, 2))
  if dof == 3: goal[:, 0, 2] = np.pi / 2
  th = O.straight_line_trajb(start[:, :, :dof], goal[:, :, :dof], 10.0, n - 1, dof)
  bt.th, bt.start, bt.goal = PC.rnd(th, 'f32'), PC.rnd(start, 'f32'), PC.rnd(goal, 'f32')
  bt.sdf = PC.rnd(O.circles_sdf(G_, O.C2_CIRCLES)[None, None], 'f32')
  bt.qc = bt.ow = bt.eps = None; bt.q_full = False
  bt.dof, bt.B, bt.n, bt.lpt, bt.c, bt.nan_rows, bt.th_clean = dof, B, n, 16, 4, np.zeros(0, np.int64), bt.th
  bt.waves = -(-B // 4)
  bt.tag = '%s B %d n %d' % (name, B, n)
  return bt


def headline(be, bt, io, K=10, nthreads=16, report=None):
  """Part 3: dgp_gn_solve_traced for K iterations (tol_delta 0 and one that mixes iteration counts) == dgp_gn_solve bit for bit; teacher forcing
  (the C oracle's step from hist[k] == hist[k+1] - hist[k], th_out for the last); the final trajectory against K untethered C-oracle steps under
  the same stopping rule, trajectories whose hinge set differs at some iteration counted and excluded; for fp32 I/O, K chained dgp_gn_step
  launches (fp32 trajectory between them) against the fused loop -> failures"""
  from oracle import blocktri as BT
  bad = []
  rep = {} if report is None else report
  p, B = bt.p, bt.B
  okw_ = dict(qc=None, ow=None, eps=None, q_full=False)
  thmax = np.abs(bt.th).reshape(B, -1).max(1)
  # the untethered oracle, tol_delta 0, and the norms that choose the mixing tol_delta (the median third-iteration norm)
  cur = bt.th.copy(); chain = [cur.copy()]; nrms = []
  for k in range(K):
    dd = BT.gn_step(p, cur, bt.start, bt.goal, bt.sdf, nthreads=nthreads)[0]
    nrms.append(np.sqrt((dd.reshape(B, -1) ** 2).sum(1))); cur = cur + dd; chain.append(cur.copy())
  tol_mix = median_tol(chain[3] - chain[2])
  for tol in (0.0, tol_mix):
    t = '%s [%s] tol_delta %.3g: ' % (bt.tag, io, tol)
    tho, its, hist, info = be.solve_traced(p, bt.th, bt.start, bt.goal, bt.sdf, K, tol, io=io)
    ref = be.solve(p, bt.th, bt.start, bt.goal, bt.sdf, K, tol, io=io)
    if not (np.array_equal(tho, ref[0]) and np.array_equal(its, ref[1])): bad.append(t + 'traced loop differs from the plain loop')
    if info.any(): bad.append(t + 'info %d trajectories' % info.astype(bool).sum())
    # teacher forcing
    worst = 0.0
    # (scale of each step: max|dtheta_b|, floored where the trajectory's own rounding dominates -- the float64 history carries eps |th| in the
    #  difference of two entries, th_out of fp32 I/O 2^-23 |th|: the floor keeps that rounding at half the tolerance)
    floor = thmax * (1e-6 if io == 'f64' else 2.0 ** -23 * 2 / PC.TOL['f32'])
    for k in range(K):
      on = its > k
      if not on.any(): break
      thk = hist[k][on]
      dk = BT.gn_step(p, thk, bt.start[on], bt.goal[on], bt.sdf, nthreads=nthreads)[0]
      last = its[on] == k + 1
      nxt = np.where((its[on] > k + 1)[:, None, None], hist[min(k + 1, K - 1)][on], 0.0)
      nxt = np.where(last[:, None, None], tho[on], nxt)      # (the last step lands in th_out)
      e = np.abs(nxt - thk - dk).reshape(on.sum(), -1).max(1) / np.maximum(np.abs(dk).reshape(on.sum(), -1).max(1), floor[on])
      worst = max(worst, float(e.max()))
      for b in np.nonzero(~(e < PC.TOL[io]))[0][:3]: bad.append(t + 'teacher forcing iteration %d: %s rel err %.3g' % (k, _where(bt, np.nonzero(on)[0][b]), e[b]))
    rep['teacher_worst_%s_%g' % (io, tol)] = worst
    # untethered: K oracle steps under the same stopping rule
    if tol == 0.0:
      o_tho, o_its, near = chain[K], np.full(B, K), np.zeros(B, bool)
    else:
      o_tho, o_its, near = stopping(bt, okw_, tol, K, nthreads, 1e-6)
    graze = np.zeros(B, bool)
    o_cur = bt.th.copy(); o_on = np.ones(B, bool)
    for k in range(K):
      on = (its > k) & (o_its > k)
      hk = np.where(on[:, None, None], hist[k], bt.th)
      ck = chain[k] if tol == 0.0 else None
      if ck is None: break
      graze |= on & (hinge_active(p, bt.sdf, hk) != hinge_active(p, bt.sdf, ck)).any(1)
    if tol != 0.0:      # (the stopping-rule chain: hinge sets compared along the kernel's own history against the oracle's chain of the same length)
      cur = bt.th.copy(); act = np.ones(B, bool)
      for k in range(K):
        on = act & (its > k)
        graze |= on & (hinge_active(p, bt.sdf, np.where(on[:, None, None], hist[k], cur)) != hinge_active(p, bt.sdf, cur)).any(1)
        dd = BT.gn_step(p, cur, bt.start, bt.goal, bt.sdf, nthreads=nthreads)[0]
        nr = np.sqrt((dd.reshape(B, -1) ** 2).sum(1))
        cur = np.where(act[:, None, None], cur + dd, cur); act &= ~(nr < tol)
    keep = ~graze & ~near & (its == o_its)
    e = np.abs(tho - o_tho).reshape(B, -1).max(1) / thmax
    rep['grazing_%s_%g' % (io, tol)] = int(graze.sum()); rep['near_tol_%s_%g' % (io, tol)] = int(near.sum())
    rep['untethered_worst_%s_%g' % (io, tol)] = float(e[keep].max()) if keep.any() else 0.0
    rep['iters_%s_%g' % (io, tol)] = sorted(set(its.tolist()))
    if (~keep & ~graze & ~near).any(): bad.append(t + '%d trajectories stop at another iteration than the oracle' % (~keep & ~graze & ~near).sum())
    tol_u = UNTETHERED_TOL[(bt.tag.split()[0], io)]
    for b in np.nonzero(keep & ~(e < tol_u))[0][:3]: bad.append(t + 'untethered: %s rel err %.3g' % (_where(bt, b), e[b]))
  if io == 'f32' and bt.tag.startswith('configs[1]'):      # K chained fp32 launches (the trajectory rounded to fp32 between them, as a torch loop over PlanLayer.forward holds it) against the fused loop
    tho, _, hist, _ = be.solve_traced(p, bt.th, bt.start, bt.goal, bt.sdf, K, 0.0, io='f32')
    cur = bt.th; graze = np.zeros(B, bool)
    for k in range(K):
      graze |= (hinge_active(p, bt.sdf, cur) != hinge_active(p, bt.sdf, hist[k])).any(1)
      dk = be.step(p, cur, bt.start, bt.goal, bt.sdf, io='f32')[0]
      ok_ = BT.gn_step(p, cur, bt.start, bt.goal, bt.sdf, nthreads=nthreads)[0]
      for b in np.nonzero(~(per_traj_rel(dk, ok_) < PC.TOL['f32']))[0][:3]: bad.append('%s chained fp32 step %d against the C oracle: %s' % (bt.tag, k, _where(bt, b)))
      cur = PC.rnd(cur + dk, 'f32')
    e = np.abs(cur - tho).reshape(B, -1).max(1) / thmax
    e[graze] = 0.0
    rep['chained_f32_grazing'] = int(graze.sum()); rep['chained_f32_worst'] = float(e.max())
    for b in np.nonzero(~(e < CHAIN_F32_TOL))[0][:3]: bad.append('%s chained fp32 steps against the fused loop: %s rel err %.3g' % (bt.tag, _where(bt, b), e[b]))
  return bad
