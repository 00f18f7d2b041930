"""numpy restatement of dgp_sdf_lookup / dgp_sdf_lookup_backward as include/dgpmp2_hip.h states them, float64, every operation in the header's order.

forward   oracle.gpmp2_oracle.bilinear_interpolate (pinned bit for bit to the reference by tests/test_oracle_golden.py) plus the summary columns;
backward  the header's closed form: g_points, the four tap contributions of every point with their cells, the dense grid gradient accumulated in point order,
          and what the bounds of the tests need: per element the sum of the absolute values of the terms of its expression, per cell the contributions it receives.
`io='f32'`: the oracle on the float32-valued inputs, every output cast once to float32 (returned widened to float64)."""
import numpy as np

from oracle import gpmp2_oracle as O

U64, U32 = 2.0 ** -53, 2.0 ** -24
NAMES = ('solved', 'num_blocked', 'first_blocked', 'min_dist', 'min_index')
# roundings on the longest path of an expression tree (see tests/test_lookup_oracle.py): a point gradient, a tap contribution
R_POINT, R_TAP = 7, 4


def lpt(S):
  """lanes per batch row of the forward kernel (dgp_host::dense_lpt)"""
  return 16 if S <= 64 else (32 if S <= 128 else 64)


def _io(a, io):
  a = np.asarray(a, np.float64)
  return a if io == 'f64' else a.astype(np.float32).astype(np.float64)


def _per_sample(grid, B):
  grid = np.asarray(grid, np.float64)
  if grid.ndim == 2: grid = grid[None]
  return np.broadcast_to(grid, (B,) + grid.shape[1:]) if grid.shape[0] == 1 else grid


def summary(d, clearance):
  """d (B, S) float64 before rounding -> (B, 5) float64"""
  B, S = d.shape
  out = np.zeros((B, len(NAMES)))
  for b in range(B):
    hit = d[b] <= clearance                       # a NaN does not block
    cnt = int(hit.sum())
    nan = np.isnan(d[b])
    mi = int(np.argmax(nan)) if nan.any() else int(np.argmin(d[b]))      # a NaN wins; the smallest index among equals
    out[b] = (0.0 if cnt else 1.0, cnt, int(np.argmax(hit)) if cnt else -1.0, d[b, mi], mi)
  return out


def distance(grid, pts, res, x_lims, y_lims, io='f64'):
  """d (B, S) in float64 BEFORE it is rounded to io: what the summary reads (and where a clearance that ties comes from)"""
  pts = _io(pts, io)[:, :, :2]
  return O.bilinear_interpolate(_per_sample(_io(grid, io), pts.shape[0]), pts, res, x_lims, y_lims)[0][:, :, 0]


def forward(grid, pts, res, x_lims, y_lims, clearance=None, io='f64'):
  """grid (B | 1, H, W) or (H, W), pts (B, S, >= 2) -> d_obs (B, S), J (B, S, 2) rounded to io, summary (B, 5) (None without a clearance)"""
  pts = _io(pts, io)[:, :, :2]
  B = pts.shape[0]
  d, J = O.bilinear_interpolate(_per_sample(_io(grid, io), B), pts, res, x_lims, y_lims)
  d = d[:, :, 0]
  return _io(d, io), _io(J, io), (None if clearance is None else summary(d, clearance))


def cell_terms(grid, pts, res, x_lims, y_lims):
  """address, taps and weights of every point, flat over (B S): the header's symbols"""
  B, S, _ = pts.shape
  H, W = grid.shape[-2:]
  ox = (0. - x_lims[0] / res)
  oy = (0. - y_lims[0] / res)
  px = (ox + pts[:, :, 0] / res).reshape(-1)
  py = (oy - pts[:, :, 1] / res).reshape(-1)
  x1 = np.floor(px).astype(np.int64); x2 = x1 + 1
  y1 = np.floor(py).astype(np.int64); y2 = y1 + 1
  x1 = np.clip(x1, 0, W - 1); x2 = np.clip(x2, 0, W - 1)
  y1 = np.clip(y1, 0, H - 1); y2 = np.clip(y2, 0, H - 1)
  pz = np.repeat(np.arange(B), S)
  g = _per_sample(grid, B)
  c = dict(pz=pz, x1=x1, x2=x2, y1=y1, y2=y2, a=g[pz, y1, x1], b=g[pz, y1, x2], c=g[pz, y2, x1], e=g[pz, y2, x2])
  c['wja'] = y2.astype(np.float64) - py; c['wjb'] = py - y1.astype(np.float64)
  c['wjc'] = x2.astype(np.float64) - px; c['wjd'] = px - x1.astype(np.float64)
  return c


def backward(grid, pts, res, x_lims, y_lims, g_d=None, g_J=None, io='f64', shared=False, wide=False):
  """-> dict: g_points (B, S, 2) rounded to io; taps_cell (B S, 4) flat cell index y W + x of a, b, c, e; taps_grid (B S,) the grid each point adds to (0 when shared);
  taps_val (B S, 4) the contributions as they are added (rounded to io unless `wide` or io is f64); g_sdf (G, H, W) their sum in point order (float64 arithmetic);
  count / abs_sum (G, H, W): contributions per cell and the sum of their absolute values; abs_points (B, S, 2) / abs_taps (B S, 4): the sum of the absolute
  values of the terms of each expression (the unit of the rounding bounds)."""
  pts = _io(pts, io)[:, :, :2]
  grid = _io(grid, io)
  B, S, _ = pts.shape
  H, W = grid.shape[-2:]
  q = cell_terms(grid, pts, res, x_lims, y_lims)
  a, b, c, e, wja, wjb, wjc, wjd = (q[k] for k in ('a', 'b', 'c', 'e', 'wja', 'wjb', 'wjc', 'wjd'))
  gd = np.zeros(B * S) if g_d is None else _io(g_d, io).reshape(-1)
  gj = np.zeros((B * S, 2)) if g_J is None else _io(g_J, io).reshape(-1, 2)
  g0, g1 = gj[:, 0], gj[:, 1]
  cr = (((e - c) - b) + a) / res
  gpx = gd * (wja * (b - a) + wjb * (e - c)) + g1 * cr
  gpy = gd * (wjc * (c - a) + wjd * (e - b)) - g0 * cr
  g_points = np.stack([gpx / res, -(gpy / res)], -1).reshape(B, S, 2)
  ta = gd * (wjc * wja) + (g0 * wja - g1 * wjc) / res
  tb = gd * (wjd * wja) - (g0 * wja + g1 * wjd) / res
  tc = gd * (wjc * wjb) + (g0 * wjb + g1 * wjc) / res
  te = gd * (wjd * wjb) + (g1 * wjd - g0 * wjb) / res
  taps = np.stack([ta, tb, tc, te], -1)
  A = np.abs
  sabs = A(a) + A(b) + A(c) + A(e)
  abs_points = np.stack([(A(gd) * (A(wja) * (A(b) + A(a)) + A(wjb) * (A(e) + A(c))) + A(g1) * sabs / res) / res,
                         (A(gd) * (A(wjc) * (A(c) + A(a)) + A(wjd) * (A(e) + A(b))) + A(g0) * sabs / res) / res], -1).reshape(B, S, 2)
  abs_taps = np.stack([A(gd * wjc * wja) + (A(g0 * wja) + A(g1 * wjc)) / res, A(gd * wjd * wja) + (A(g0 * wja) + A(g1 * wjd)) / res,
                       A(gd * wjc * wjb) + (A(g0 * wjb) + A(g1 * wjc)) / res, A(gd * wjd * wjb) + (A(g1 * wjd) + A(g0 * wjb)) / res], -1)
  vals = taps if (wide or io == 'f64') else _io(taps, 'f32')
  cells = np.stack([q['y1'] * W + q['x1'], q['y1'] * W + q['x2'], q['y2'] * W + q['x1'], q['y2'] * W + q['x2']], -1)
  tg = np.zeros(B * S, np.int64) if shared else q['pz']
  G = 1 if shared else B
  g_sdf, count, abs_sum, abs_terms = np.zeros((G, H * W)), np.zeros((G, H * W), np.int64), np.zeros((G, H * W)), np.zeros((G, H * W))
  for t in range(4):
    np.add.at(g_sdf, (tg, cells[:, t]), vals[:, t])
    np.add.at(count, (tg, cells[:, t]), 1)
    np.add.at(abs_sum, (tg, cells[:, t]), np.abs(vals[:, t]))
    np.add.at(abs_terms, (tg, cells[:, t]), abs_taps[:, t])
  sh = (G, H, W)
  return dict(g_points=_io(g_points, io), taps_cell=cells, taps_grid=tg, taps_val=vals, g_sdf=g_sdf.reshape(sh), count=count.reshape(sh), abs_sum=abs_sum.reshape(sh),
              abs_terms=abs_terms.reshape(sh), abs_points=abs_points, abs_taps=abs_taps)


def grid_bound(ref, u):
  """per cell: 0 where it receives at most one contribution (the atomic adds it to zero: exact), (K + 1) u sum|t_i| elsewhere"""
  K = ref['count']
  return np.where(K <= 1, 0.0, (K + 1) * u * ref['abs_sum'])


def per_cell_contributions(ref):
  """{(grid, y, x): [contributions in point order]} -- the list behind every cell of the grid gradient"""
  G, H, W = ref['g_sdf'].shape
  out = {}
  for p in range(ref['taps_cell'].shape[0]):
    for t in range(4):
      cidx = int(ref['taps_cell'][p, t])
      out.setdefault((int(ref['taps_grid'][p]), cidx // W, cidx % W), []).append(float(ref['taps_val'][p, t]))
  return out
