"""numpy restatement of dgp_select_samples (include/dgpmp2_hip.h): the status bits, the tier, the total order, best, th_best and the problem summary of every problem,
from tests/interp_oracle.py's dense trajectory and DGP_DENSE_* summary of each sample plus its score and exclude flag.  Every key of the order is an input or a
number the interpolation oracle gives bit for bit, so everything here is exact; th_best comes by indexing."""
import numpy as np

import interp_oracle as IO_

COLLIDING, OUTSIDE, NON_FINITE, EXCLUDED = 1, 2, 4, 8
NAMES = ('solved', 'num_accepted', 'best_index', 'best_score', 'best_max_penetration', 'best_status')
COL = {k: i for i, k in enumerate(NAMES)}
MAXP, NUMC = IO_.COL['max_penetration'], IO_.COL['num_colliding']


class Result(object):
  """status, tier, order (B,S) int; best (B) int; th_best (B,n,d); sample_summary (B,S,6) or None; problem_summary (B,6); max_pen, score (B,S) float64"""
  def __init__(self, **kw): self.__dict__.update(kw)


def problem_major(a, sample_major):
  """(S,B,...) -> (B,S,...) where sample_major"""
  a = np.asarray(a)
  return np.ascontiguousarray(np.swapaxes(a, 0, 1)) if sample_major else a


def grids_per_sample(sdf, B, S, env_index=None):
  """the grid every one of the B S trajectories reads, (B S | 1, 1, H, W): sdf (1,1,H,W) shared, or (G,1,H,W) with problem b on grid env_index[b] (None: grid b)"""
  sdf = np.asarray(sdf)
  if sdf.shape[0] == 1 and env_index is None: return sdf
  env = np.arange(B) if env_index is None else np.asarray(env_index)
  return np.repeat(sdf[env], S, axis=0)


def run(p, th, K, sdf=None, eps=0.0, score=None, exclude=None, require_inside=True, sample_major=False, env_index=None, io='f64'):
  """what the kernel must give.  th (B,S,n,d) -- (S,B,n,d) with sample_major, like score and exclude -- of numbers exact in `io`."""
  rnd = (lambda a: a) if io == 'f64' else (lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64))
  th = problem_major(np.asarray(th, np.float64), sample_major)
  B, S, n, d = th.shape
  flat = th.reshape(B * S, n, d)
  sc = np.zeros((B, S)) if score is None else rnd(problem_major(np.asarray(score, np.float64), sample_major))
  ex = np.zeros((B, S), np.int64) if exclude is None else problem_major(exclude, sample_major).astype(np.int64)
  d64 = IO_.dense(p, flat, K)                                   # the unrounded positions the lookup takes (copies: the stored values)
  x, y = d64[:, :, 0], d64[:, :, 1]
  with np.errstate(invalid='ignore'):
    inside = (x >= p.x_lims[0]) & (x <= p.x_lims[1]) & (y >= p.y_lims[0]) & (y <= p.y_lims[1])      # a NaN is outside
  outside = (~inside).any(1).reshape(B, S)
  summ = None
  if sdf is not None:
    summ = IO_.summary(IO_.cost(p, d64, grids_per_sample(sdf, B, S, env_index), eps)).reshape(B, S, len(IO_.NAMES))
  max_pen = summ[:, :, MAXP] if summ is not None else np.zeros((B, S))
  colliding = summ[:, :, NUMC] != 0 if summ is not None else np.zeros((B, S), bool)
  non_finite = ~np.isfinite(flat).all((1, 2)).reshape(B, S) | ~np.isfinite(sc) | np.isnan(max_pen)
  excluded = ex != 0
  status = colliding * COLLIDING + outside * OUTSIDE + non_finite * NON_FINITE + excluded * EXCLUDED
  tier = np.where(non_finite | excluded, 2, np.where(colliding | (bool(require_inside) & outside), 1, 0))
  order = np.empty((B, S), np.int64)
  for b in range(B):
    key = lambda s: (int(tier[b, s]), float(max_pen[b, s]) if tier[b, s] == 1 else 0.0, float(sc[b, s]) if tier[b, s] < 2 else 0.0, s)      # (-0.0 == 0.0: a tie)
    order[b] = sorted(range(S), key=key)
  best = order[:, 0]
  rows = np.arange(B)
  ps = np.zeros((B, len(NAMES)))
  ps[:, COL['solved']] = tier[rows, best] == 0
  ps[:, COL['num_accepted']] = (tier == 0).sum(1)
  ps[:, COL['best_index']] = best
  ps[:, COL['best_score']] = sc[rows, best]
  ps[:, COL['best_max_penetration']] = max_pen[rows, best]
  ps[:, COL['best_status']] = status[rows, best]
  return Result(status=status.astype(np.int64), tier=tier.astype(np.int64), order=order, best=best, th_best=th[rows, best], sample_summary=summ, problem_summary=ps,
                max_pen=max_pen, score=sc)
