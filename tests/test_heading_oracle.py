"""dgp_heading_lift without a GPU: tests/heading_oracle.py (the numpy restatement of include/dgpmp2_hip.h that tests/test_hip_heading.py holds the kernel against)
checked against the reference's own straight_line_trajb with dof = 3 (fixture g14_heading_lift, bit for bit) and against the invariants the tangent rule was made for;
the torch mirror utils.planner_utils.heading_lift_torch against the oracle, bit for bit with the turns passed in; the export line; the host-side argument
validation of the entry point (a call that fails it launches nothing, so it runs without a device).

The bounds.  theta_N = phi_N + wrap(theta_g - phi_N) is congruent to theta_g up to the roundings of the difference, of the quotient's multiple TWO_PI * k, of the
subtraction and of the final sum: four roundings of at most half an ulp of the largest magnitude among them, M = max(|theta_g|, |phi_N|, |TWO_PI k|, |theta_N|): the
residual, formed exactly in rational arithmetic, is held to 4 ulp(M) -- the issue's bound.  On a circular arc sampled at equal angles the chord P_(i+1) - P_(i-1) is
exactly perpendicular to the radius at P_i, and phi_i is the direction of that chord summed from turns of a few ulp each: |vy cos(theta) - vx sin(theta)| / |v| is the
sine of an angle error of at most (i + 2) 3 ulp(pi) ~ 1e-13 at n = 64, inside 1e-12.  With the default blend >= 4 rows and both end errors at most pi, one row changes a
blend term by at most pi / 4 each, so between rows whose turn is at most pi / 2 (info bit 2 clear) the heading moves by at most pi / 2 + pi / 4 + pi / 4 = pi."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import heading_cases as HC
import heading_oracle as HO
import problems_oracle as PR
from dgpmp2_amd import _capi
from dgpmp2_amd.utils import planner_utils as PU

NS = (2, 3, 17, 64, 65, 130)
END_MODES = ('supplied', 'random', 'tangent', ('tangent', 'supplied'), ('random', 'tangent'))


def ulp(v): return float(np.spacing(np.abs(np.float64(v))))


def test_linear_keep_is_the_reference_straight_line(golden):
  g = golden('g14_heading_lift')
  assert len(g['cases']) >= 5
  for k, c in enumerate(g['cases']):
    n, T = int(c.split()[0]), float(g['c%d_T' % k])
    s, go, want = g['c%d_start' % k], g['c%d_goal' % k], g['c%d_th' % k]
    assert want.shape == (s.shape[0], n, 6)
    th2 = np.stack([PR.straight_line(s[b, 0, :2], go[b, 0, :2], n, T) for b in range(s.shape[0])])
    start, goal, th, turns, info = HO.run(th2, T, 'linear', 'supplied', 'keep', 1, s[:, 0, 2], go[:, 0, 2])
    assert HC.same_bits(th, want), (c, np.abs(th - want).max())
    assert HC.same_bits(start[:, 0, :3], want[:, 0, :3]) and HC.same_bits(goal[:, 0, :3], want[:, -1, :3]) and not start[:, 0, 3:].any() and not goal[:, 0, 3:].any()
    assert not turns.any() and not info.any()
    # the torch mirror as well
    t = PU.heading_lift_torch(torch.from_numpy(th2), T, torch.from_numpy(s[:, 0, 2].copy()), torch.from_numpy(go[:, 0, 2].copy()), 'linear', 'supplied', 'keep', 1)
    assert HC.same_bits(t[2].numpy(), want)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_torch_mirror_equals_the_oracle_with_the_turns_passed_in(io):
  seen = set()
  tdt = np.float32 if io == 'f32' else np.float64
  for n in NS:
    N = n - 1
    th2, _ = HC.batch(n, len(HC.KINDS), 0, io)
    B = th2.shape[0]
    hs, hg = HC.headings(B, n)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for heading in ('tangent', 'linear'):
      for ends in END_MODES:
        if heading == 'linear' and 'tangent' in ((ends,) if isinstance(ends, str) else ends): continue
        for velocity in ('diff', 'keep'):
          for blend in sorted({1, min(3, N), N}):
            gen = HO.run(th2, HC.T_SEC, heading, ends, velocity, blend, hs, hg, None, 5, 7, io)
            want = HO.run(th2, HC.T_SEC, heading, ends, velocity, blend, hs, hg, gen[3], 5, 7, io)
            assert all(HC.same_bits(a, b) for a, b in zip(want[:4], gen[:4])) and np.array_equal(want[4], gen[4])      # the oracle's own turns fed back
            got = PU.heading_lift_torch(T(th2.astype(tdt)), HC.T_SEC, T(hs), T(hg), heading, ends, velocity, blend, 5, 7, T(gen[3]))
            tag = (io, n, heading, ends, velocity, blend)
            assert got[2].dtype == T(th2.astype(tdt)).dtype and got[4].dtype == torch.int32
            assert all(HC.same_bits(a.numpy().astype(np.float64), b) for a, b in zip(got[:4], want[:4])), tag
            assert np.array_equal(got[4].numpy(), want[4]), tag
            seen |= set(want[4].tolist())
            # without them: torch's atan2 against numpy's, far inside the rounding of the output
            own = PU.heading_lift_torch(T(th2.astype(tdt)), HC.T_SEC, T(hs), T(hg), heading, ends, velocity, blend, 5, 7)
            fin = np.isfinite(want[2])
            assert np.array_equal(np.isfinite(own[2].numpy()), fin) and np.abs(own[2].numpy().astype(np.float64)[fin] - want[2][fin]).max() <= (1e-9 if io == 'f64' else 1e-4), tag
  bits = 0
  for v in seen: bits |= v
  assert bits == 15 and 0 in seen      # every info bit occurs, and clean trajectories too


def test_invariants_of_the_tangent_lift():
  for n in (17, 64, 130):
    N = n - 1
    blend = max(1, N // 4)
    th2, names = HC.batch(n, len(HC.KINDS), 0)
    hs, hg = HC.headings(len(names), 3 * n)
    start, goal, th, turns, info = HO.run(th2, HC.T_SEC, 'tangent', 'supplied', 'diff', blend, hs, hg)
    for b, name in enumerate(names):
      if info[b] & HO.NON_FINITE: continue
      assert th[b, 0, 2] == hs[b] == start[b, 0, 2] and goal[b, 0, 2] == th[b, N, 2], name      # theta_0 is theta_s itself
      k = round((Fraction(th[b, N, 2]) - Fraction(hg[b])) / Fraction(HO.TWO_PI))
      resid = abs(Fraction(th[b, N, 2]) - Fraction(hg[b]) - k * Fraction(HO.TWO_PI))
      M = max(abs(hg[b]), abs(th[b, N, 2]), abs(HO.TWO_PI * k), abs(th[b, N, 2] - (th[b, N, 2] - hg[b])))
      assert resid <= 4 * Fraction(ulp(M)), (name, n, float(resid), ulp(M))
      if not info[b] & HO.SHARP_TURN:
        assert np.abs(np.diff(th[b, :, 2])).max() <= HO.PI * (1 + 1e-15), (name, n)
    # the kinds of the cases come out as their flags
    flags = dict(zip(names, info.tolist()))
    assert flags['arc'] == 0 and flags['s_curve'] == 0 and flags['staircase'] == 0
    assert flags['corner'] == 0 and flags['reversal'] == HO.SHARP_TURN | HO.FILLED      # central differences split a corner over two rows: only a reversal turns by more than a right angle at once
    assert flags['repeated_front'] == HO.FILLED and flags['repeated_middle'] & HO.FILLED
    assert flags['repeated_everywhere'] == HO.ALL_DEGENERATE | HO.FILLED and flags['non_finite'] & HO.NON_FINITE and flags['non_finite'] & HO.FILLED
    # a path that never moves: every heading follows (1, 0), blended into the ends
    e = names.index('repeated_everywhere')
    assert not turns[e].any() and not th[e, :, 3:5].any()
    # the reversal turns by +pi exactly once
    r = names.index('reversal')
    assert (np.abs(turns[r, 1:]) > 3.0).sum() == 1 and turns[r, 1:].max() == np.pi
    # tangent ends on a circular arc: the non-holonomic error vanishes on interior rows, and theta is the tangent direction everywhere
    arc = th2[names.index('arc')][None]
    th_a = HO.run(arc, HC.T_SEC, 'tangent', 'tangent', 'diff', blend)[2][0]
    vx, vy, theta = th_a[1:N, 3], th_a[1:N, 4], th_a[1:N, 2]
    err = np.abs(vy * np.cos(theta) - vx * np.sin(theta))
    assert (err <= 1e-12 * np.sqrt(vx * vx + vy * vy)).all(), (n, (err / np.sqrt(vx * vx + vy * vy)).max())
    # both ends tangent: theta_i = phi_i, no blend term
    both = HO.run(th2, HC.T_SEC, 'tangent', 'tangent', 'diff', 1)
    again = HO.run(th2, HC.T_SEC, 'tangent', 'tangent', 'diff', N)
    assert HC.same_bits(both[2], again[2])


def test_random_ends_are_a_function_of_seed_and_problem():
  th2, _ = HC.batch(17, 5, 0)
  a = HO.run(th2, HC.T_SEC, 'tangent', 'random', 'diff', 4, seed=9, first_problem=100)
  b = HO.run(th2[2:], HC.T_SEC, 'tangent', 'random', 'diff', 4, seed=9, first_problem=102)
  assert HC.same_bits(a[2][2:], b[2]) and HC.same_bits(a[0][2:], b[0])
  hs = a[0][:, 0, 2]
  assert ((hs >= -HO.PI) & (hs < HO.PI)).all() and len(set(hs.tolist())) == 5
  assert not HC.same_bits(HO.run(th2, HC.T_SEC, 'tangent', 'random', 'diff', 4, seed=10, first_problem=100)[0], a[0])
  # stream 2 of the sampler's generator, counter word 2 zero
  w = PR.philox4x32_10((100, 0, 0, 2), (9, 0))
  assert hs[0] == (-HO.PI) + float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53 * HO.TWO_PI


def test_export_line_and_build_table():
  api = _capi.get_api()
  assert 'heading_lift' in _capi.CApi.SYMBOLS and api.heading_lift is not None and api.abi_version() == 7 and _capi.DGP_ABI_VERSION == 7
  assert C.sizeof(_capi.DgpHeadingParams) == 40
  from dgpmp2_amd._build.units import UNITS
  assert any(u.name == 'heading_lift' and u.source == 'heading_lift.hip' and u.launcher is None for u in UNITS)


def _cfg(**kw):
  base = dict(num_states=17, dof=3, io_dtype=_capi.DGP_F64, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], cost_sigma=0.01, epsilon_dist=0.4, non_holonomic=True, K_d=0.01)
  base.update(kw)
  return _capi.make_config(**base)


def test_the_entry_point_validates_its_arguments_without_a_device():
  """Validation comes before anything touches a device, so every case answers DGP_EINVAL on a machine without one.  Where a device IS present, the pointers are one real
  device buffer large enough for every argument (B = 2, n = 17, fp64), so that validation gone wrong would launch on memory it may write; without a device a launch
  cannot happen, it would come back as a HIP error instead of DGP_EINVAL, and the address is a placeholder that nothing reads.  tests/test_hip_heading.py shows on the
  GPU that each case leaves every output untouched."""
  s = _capi.Solver(_cfg())
  import torch
  hold = torch.zeros(2 * 17 * 6, dtype=torch.float64, device='cuda:0') if torch.cuda.is_available() else None
  P, ok = _capi.Solver.heading_params, (hold.data_ptr() if hold is not None else 0x1000)
  L, Tn, SUP, ETAN, RND = _capi.DGP_HEADING_LINEAR, _capi.DGP_HEADING_TANGENT, _capi.DGP_END_SUPPLIED, _capi.DGP_END_TANGENT, _capi.DGP_END_RANDOM
  call = lambda solver, B, p, th2=ok, hs=ok, hg=ok, start=ok, goal=ok, th=ok: solver.heading_lift(B, p, th2, start, goal, th, hs, hg)
  bad = [
      (s, 0, P(blend=4), {}),                                                      # batch
      (s, 2, None, {}),                                                            # params
      (s, 2, P(blend=4), dict(th2=None)), (s, 2, P(blend=4), dict(start=None)), (s, 2, P(blend=4), dict(goal=None)), (s, 2, P(blend=4), dict(th=None)),
      (s, 2, P(heading_mode=2, blend=4), {}), (s, 2, P(velocity_mode=2, blend=4), {}), (s, 2, P(start_end=3, blend=4), {}), (s, 2, P(goal_end=-1, blend=4), {}),
      (s, 2, P(blend=0), {}), (s, 2, P(blend=17), {}),                             # blend outside 1 .. N = 16
      (s, 2, P(L, ETAN, SUP, blend=4), {}), (s, 2, P(L, SUP, ETAN, blend=4), {}),  # tangent ends under the linear rule
      (s, 2, P(Tn, SUP, RND, blend=4), dict(hs=None)), (s, 2, P(Tn, RND, SUP, blend=4), dict(hg=None)),      # supplied ends without their arrays
      (_capi.Solver(_cfg(dof=2, Q_c_inv=[[1, 0], [0, 1]], non_holonomic=False, K_d=0.0)), 2, P(blend=4), {}),      # a planar handle
  ]
  for solver, B, p, kw in bad:
    with pytest.raises(_capi.DgpError) as e:
      call(solver, B, p, **kw)
    assert e.value.code == _capi.DGP_EINVAL and len(str(e.value)) > 20, (B, kw)
  with pytest.raises(_capi.DgpError):
    s.api.check(s.api.heading_lift(None, 2, C.byref(P(blend=4)), ok, ok, ok, None, ok, ok, ok, None, None, None))      # the handle
  if hold is not None:
    torch.cuda.synchronize()
    assert not bool(hold.any())      # and nothing wrote the buffer
