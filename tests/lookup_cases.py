"""Inputs of the SDF-lookup tests (dgp_sdf_lookup / dgp_sdf_lookup_backward), shared by the CPU tests, the GPU tests and tests/golden/make_lookup_golden.py.

Grids: 5 x 7 and 2 x 2 of multiples of 1/1024, and the four 40 x 32 signed-distance fields of fixture g1_factors_2d.  A FRAME is (res, x_lims, y_lims): the 40 x 32
grids are looked up at the padded-width resolution 10 / 32 and at the cell size 10 / 30 a caller of check_solved takes from im_size; 5 x 7 at 10 / 7 (not a dyadic
number: x / res rounds), 2 x 2 at 5.
Points of a (B, S) batch cycle through nine kinds by their flat index: interior; exactly on a cell line (integer px and py); in the last column cell; in the last
row cell; outside the left / right / top / bottom side (clamped cells: coinciding taps); at +-1e6.  Everything is float64; the float32 runs cast it."""
import os

import numpy as np

X_LIMS, Y_LIMS = (-5.0, 5.0), (-5.0, 5.0)
KINDS = ('interior', 'on_lines', 'last_col', 'last_row', 'left', 'right', 'top', 'bottom', 'far')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def bits(a):
  return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b):
  """bit for bit, any NaN equal to any NaN"""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def as_io(a, io):
  """the float64 array holding what a buffer of `io` holds"""
  return np.asarray(a, np.float64) if io == 'f64' else np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def grids(name, count):
  """-> (count, H, W) float64"""
  if name == 'g1':
    g = np.load(os.path.join(GOLDEN, 'g1_factors_2d.npz'))['sdf'][:, 0]
    return np.ascontiguousarray(g[np.arange(count) % g.shape[0]] + 0.03125 * (np.arange(count) // g.shape[0])[:, None, None])
  H, W = {'5x7': (5, 7), '2x2': (2, 2)}[name]
  rs = np.random.RandomState(H * 100 + W)
  return rs.randint(-2048, 2049, (count, H, W)).astype(np.float64) / 1024.0


# name -> (grid name, res)
FRAMES = {'g1': ('g1', 10.0 / 32), 'g1_cell': ('g1', 10.0 / 30), '5x7': ('5x7', 10.0 / 7), '2x2': ('2x2', 5.0)}


def pixel(x, y, res):
  """px, py as the header forms them"""
  return (0. - X_LIMS[0] / res) + x / res, (0. - Y_LIMS[0] / res) - y / res


def _world(px, py, res):
  return (px - (0. - X_LIMS[0] / res)) * res, ((0. - Y_LIMS[0] / res) - py) * res


def _on_line(k, res, axis):
  """a coordinate whose pixel coordinate is exactly the integer k (searched a few ulps around the inverse map), or None: at a resolution like 1 / 3 some lines
  have no such coordinate"""
  x0 = _world(float(k), float(k), res)[axis]
  cands = [x0]
  for s in range(1, 8):
    lo = hi = x0
    for _ in range(s): lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    cands += [lo, hi]
  for x in cands:
    if pixel(x, x, res)[axis] == float(k): return x
  return None


def _some_line(rs, n, res, axis):
  """a coordinate on one of the pixel lines 0 .. n - 1, the lines tried in a random order"""
  for k in rs.permutation(n):
    x = _on_line(int(k), res, axis)
    if x is not None: return x
  raise AssertionError('no pixel line of 0 .. %d can be hit exactly at res %r' % (n - 1, res))


def points(frame, B, S, seed=0):
  """-> (B, S, 2) float64"""
  gname, res = FRAMES[frame]
  H, W = grids(gname, 1).shape[1:]
  rs = np.random.RandomState(seed + 31 * B + S)
  out = np.zeros((B, S, 2))
  for f in range(B * S):
    kind = KINDS[(f + seed) % len(KINDS)]
    u, v = rs.uniform(0.05, 0.95, 2)
    if kind == 'interior': px, py = rs.uniform(0, W - 1), rs.uniform(0, H - 1)
    elif kind == 'last_col': px, py = W - 1 - (u if f % 2 else -u), rs.uniform(0, H - 1)      # [W-2, W-1) and [W-1, W): the latter has x1 = x2 = W - 1
    elif kind == 'last_row': px, py = rs.uniform(0, W - 1), H - 1 - (v if f % 2 else -v)
    elif kind == 'left': px, py = -0.5 - 3 * u, rs.uniform(0, H - 1)
    elif kind == 'right': px, py = W + 3 * u, rs.uniform(0, H - 1)
    elif kind == 'top': px, py = rs.uniform(0, W - 1), -0.5 - 3 * v
    elif kind == 'bottom': px, py = rs.uniform(0, W - 1), H + 3 * v
    else: px, py = 0.0, 0.0
    x, y = _world(px, py, res)
    if kind == 'on_lines': x, y = _some_line(rs, W, res, 0), _some_line(rs, H, res, 1)
    if kind == 'far': x, y = (1.0e6, -1.0e6) if f % 2 else (-1.0e6, 1.0e6)
    out[f // S, f % S] = x, y
  return out


def disjoint_points(frame, B, S, shared, seed=0):
  """points whose 2 x 2 footprints share no cell inside a grid (inside THE grid when it is shared): every cell of the grid gradient then receives at most one
  contribution and the atomics add to zero once -- or None where the grid has no room for that many"""
  gname, res = FRAMES[frame]
  H, W = grids(gname, 1).shape[1:]
  cells = [(x, y) for y in range(0, H - 1, 3) for x in range(0, W - 1, 3)]
  need = B * S if shared else S
  if need > len(cells): return None
  rs = np.random.RandomState(seed + 7 * B + S)
  out = np.zeros((B, S, 2))
  order = rs.permutation(len(cells))
  for b in range(B):
    if not shared: order = rs.permutation(len(cells))      # one permutation per grid; a shared grid: one for the whole batch
    for s in range(S):
      cx, cy = cells[order[b * S + s if shared else s]]
      out[b, s] = _world(cx + rs.uniform(0.1, 0.9), cy + rs.uniform(0.1, 0.9), res)
  return out


def cotangents(B, S, seed=0):
  """random cotangents on both outputs: g_d (B, S), g_J (B, S, 2), multiples of 1/256 (exact in float32)"""
  rs = np.random.RandomState(1000 + seed + 13 * B + S)
  return rs.randint(-512, 513, (B, S)).astype(np.float64) / 256.0, rs.randint(-512, 513, (B, S, 2)).astype(np.float64) / 256.0


def tile(g):
  """(B, H, W) -> the (B, ceil(H/4) * ceil(W/4) * 16) elements of DGP_SDF_TILED4 (padding cells zero)"""
  B, H, W = g.shape
  Ht, Wt = (H + 3) // 4, (W + 3) // 4
  p = np.zeros((B, Ht * 4, Wt * 4), g.dtype)
  p[:, :H, :W] = g
  return np.ascontiguousarray(p.reshape(B, Ht, 4, Wt, 4).transpose(0, 1, 3, 2, 4)).reshape(B, -1)


def untile(t, H, W):
  B = t.shape[0]
  Ht, Wt = (H + 3) // 4, (W + 3) // 4
  return np.ascontiguousarray(t.reshape(B, Ht, Wt, 4, 4).transpose(0, 1, 3, 2, 4).reshape(B, Ht * 4, Wt * 4)[:, :H, :W])
