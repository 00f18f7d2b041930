"""Inputs of the heading-lift tests (dgp_heading_lift), shared by the CPU tests, the GPU tests and nothing else: planar trajectories (n,4) -- positions in columns 0, 1,
the constant velocities of path_to_traj_avg_vel in columns 2, 3 -- of the kinds the planar chain produces and of the kinds that break a tangent."""
import numpy as np

import heading_oracle as HO

T_SEC = 10.0


def resample(vertices, n):
  """n points at equal arc length along the polyline `vertices` (k,2), the way a grid path is resampled; the last point is the last vertex itself"""
  v = np.asarray(vertices, dtype=np.float64)
  seg = np.sqrt(((v[1:] - v[:-1]) ** 2).sum(1))
  s = np.concatenate([[0.0], np.cumsum(seg)])
  out = np.empty((n, 2))
  for i in range(n):
    t = s[-1] * i / (n - 1)
    j = min(int(np.searchsorted(s[1:], t)), len(seg) - 1)
    f = (t - s[j]) / seg[j] if seg[j] > 0 else 0.0
    out[i] = v[j] + f * (v[j + 1] - v[j])
  out[-1] = v[-1]
  return out


def with_velocities(p):
  th2 = np.zeros((p.shape[0], 4))
  th2[:, :2] = p
  th2[:, 2:] = (p[-1] - p[0]) / T_SEC
  return th2


def arc(n, radius=2.5, a0=-0.4, a1=2.3, centre=(0.3, -0.2)):
  a = a0 + (a1 - a0) * np.arange(n) / max(n - 1, 1)
  return np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1)


def s_curve(n):
  x = -4.0 + 8.0 * np.arange(n) / max(n - 1, 1)
  return np.stack([x, 1.5 * np.sin(0.9 * x)], axis=1)


def staircase(n):
  """axis and diagonal moves of a 5-7 grid path, resampled"""
  v, p = [(-3.5, -3.0)], np.array([-3.5, -3.0])
  for k, step in enumerate([(1, 0), (1, 1), (1, 1), (0, 1), (1, 0), (1, 1), (0, 1), (0, 1), (1, 0), (1, 1), (1, 0)]):
    p = p + 0.5 * np.array(step, dtype=np.float64) * (1 + k % 2)
    v.append(tuple(p))
  return resample(v, n)


def corner(n):
  return resample([(-3.0, -2.0), (1.0, -2.0), (-1.0, 3.0)], n)      # one corner of 112 degrees


def reversal(n):
  """out along a line and back over the same points, in exactly representable steps: the tangent at the turning point is zero (filled) and the next one exactly
  antiparallel -- a turn of +pi"""
  s = np.array([min(i, 2 * (n // 2) - i) for i in range(n)], dtype=np.float64)
  return np.stack([-3.0 + s / 64.0, -1.0 + s / 128.0], axis=1)


def repeated_front(n):
  p = arc(n)
  p[:max(1, n // 3)] = p[max(1, n // 3)] if n > 2 else p[0]
  return p


def repeated_middle(n):
  p = s_curve(n)
  a, b = n // 3, max(n // 3 + 1, (2 * n) // 3)
  p[a:b] = p[a]
  return p


def repeated_everywhere(n):
  return np.tile(np.array([[1.25, -0.75]]), (n, 1))


def non_finite(n):
  p = s_curve(n)
  p[n // 2, 1] = np.nan
  return p


KINDS = (('arc', arc), ('s_curve', s_curve), ('staircase', staircase), ('corner', corner), ('reversal', reversal), ('repeated_front', repeated_front),
         ('repeated_middle', repeated_middle), ('repeated_everywhere', repeated_everywhere), ('non_finite', non_finite))
DEGENERATE = ('reversal', 'repeated_front', 'repeated_middle', 'repeated_everywhere', 'non_finite')      # the kinds with a degenerate tangent


def case(name, n, io='f64'):
  """-> th2 (n,4) float64 holding io-rounded values"""
  return HO.rnd(with_velocities(dict(KINDS)[name](n)), io)


def batch(n, B, first=0, io='f64'):
  """B trajectories, the kinds in turn from `first` on -> th2 (B,n,4), names"""
  names = [KINDS[(first + b) % len(KINDS)][0] for b in range(B)]
  return np.stack([case(k, n, io) for k in names]), names


def headings(B, seed):
  """supplied end headings, some far outside (-pi, pi]"""
  rs = np.random.RandomState(seed)
  return rs.uniform(-7.0, 7.0, B), rs.uniform(-7.0, 7.0, B)


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
  """equal as bit patterns, every NaN equal to every NaN"""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())
