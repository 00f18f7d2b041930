"""CPU-only tests of the problem sampler's oracle and of the host side of dgp_sample_problems.

  * tests/problems_oracle.py against the reference's own verdicts (tests/golden/g10_problems.npz, made by tests/golden/make_problems_golden.py from Env2D.is_feasible
    and straight_line_trajb): feasibility exactly -- pixel centres, the last row and column, the limits, points outside them, clearances 5e-13 either side of a point's
    own distance -- and the initial trajectories bit for bit;
  * its Philox4x32-10 against the known-answer vectors published with Random123;
  * the inputs of the GPU tests (tests/problems_cases.py) take every branch the sampler has;
  * argument validation of dgp_sample_problems (nothing touches a device), the struct layout and the Python front end's refusal of host tensors."""
import ctypes as C
import os

import numpy as np
import pytest

import problems_cases as PCS
import problems_oracle as PO
from dgpmp2_amd import _capi


def test_feasibility_equals_the_reference(golden):
  g = golden('g10_problems')
  total = 0
  for f in g['fields']:
    sdf, pts, clear, want, dist = g[f + '_sdf'], g[f + '_points'], g[f + '_clearances'], g[f + '_feasible'], g[f + '_dist']
    got_d = np.array([PO.signed_distance(sdf, p[0], p[1], (-5.0, 5.0), (-5.0, 5.0)) for p in pts])
    got = np.array([PO.is_feasible(sdf, p[0], p[1], c) for p, c in zip(pts, clear)])
    assert np.array_equal(got_d, dist), f      # bit for bit: the verdicts at a clearance 5e-13 away hang on it
    assert np.array_equal(got, want), f
    outside = np.abs(pts).max(1) > 5.0
    assert outside.sum() >= 8 and (got_d[outside] == 10.0).all() and want[outside & (clear < 10.0)].all()      # MAX_D: feasible at any smaller clearance
    assert (np.abs(clear - dist) < 1e-12).sum() >= 20 and want.any() and not want.all()
    total += len(pts)
  assert total >= 200


def test_last_column_and_row_follow_the_clamped_taps(golden):
  """The reference forms the bilinear weights from the CLAMPED upper indices (env_2d.py:133-147): on the last column / row both taps coincide, the two weights cancel and
  the distance collapses to (nearly) zero -- infeasible at any positive clearance, however free the cell is.  The fixture pins that."""
  g = golden('g10_problems')
  sdf = g['circles_sdf']
  W = sdf.shape[1]
  x = 5.0 - 0.25 * 10.0 / W
  assert sdf[4, W - 1] > 1.0 and abs(PO.signed_distance(sdf, x, 5.0 - 4.5 * 10.0 / W, (-5.0, 5.0), (-5.0, 5.0))) < 1e-9
  pts, dist = g['circles_points'], g['circles_dist']
  last = (pts[:, 0] > 5.0 - 10.0 / W) & (pts[:, 0] <= 5.0) & (np.abs(pts[:, 1]) <= 5.0)
  assert last.sum() >= 8 and np.all(np.abs(dist[last]) < 1e-9)


def test_initial_trajectories_equal_the_reference_bit_for_bit(golden):
  g = golden('g10_problems')
  for n in (3, 16, 64):
    want = g['line_th_n%d' % n]
    got = PO.th_init_of(g['line_start'], g['line_goal'], n, float(g['total_time_sec']))
    assert got.dtype == np.float64 and np.array_equal(got, want), n
  # the repository's own straight_line_trajb is the same function
  from oracle.gpmp2_oracle import straight_line_trajb
  assert np.array_equal(straight_line_trajb(g['line_start'][:, :, :2], g['line_goal'][:, :, :2], 10.0, 15, 2), g['line_th_n16'])


def test_philox_known_answers():
  """The known-answer vectors of Random123's kat_vectors for philox4x32 with 10 rounds (counter, key -> output): all zeros, all ones, and the digits of pi.  The
  all-zero vector -- 6627e8d5 e169c58d bc57ac4c 9b00dbd8 -- and an arbitrary counter / key were also confirmed against a second implementation, the Philox4_32 engine
  of torch's ATen headers (ATen/core/PhiloxRNGEngine.h, compiled on the host: engine(seed, subsequence, offset) has key = seed, counter = (offset, subsequence))."""
  h = lambda w: ' '.join('%08x' % v for v in w)
  assert h(PO.philox4x32_10((0, 0, 0, 0), (0, 0))) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
  m = 0xffffffff
  assert h(PO.philox4x32_10((m, m, m, m), (m, m))) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
  assert h(PO.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == 'd16cfe09 94fdcceb 5001e420 24126ea1'
  assert h(PO.philox4x32_10((5, 0, 7, 0), (0x89abcdef, 0x01234567))) == '414da380 b7702af1 cd642c43 43dc5e58'      # at::Philox4_32(0x0123456789abcdef, 7, 5)


def test_candidates_are_uniform_in_the_box_and_counter_based():
  P = PCS.params()
  pts = np.array([PO.candidate(P, 3, 5, k, s) for k in range(400) for s in (0, 1)])
  assert pts.min() >= -4.5 and pts.max() < 4.5 and abs(pts.mean()) < 0.3 and len({tuple(p) for p in pts}) == 800
  assert PO.candidate(P, 3, 5, 9, 0) != PO.candidate(P, 3, 5, 9, 1) and PO.candidate(P, 3, 5, 9, 0) != PO.candidate(P, 4, 5, 9, 0)
  assert PO.candidate(P, 3, (1 << 40) + 5, 9, 0) != PO.candidate(P, 3, 5, 9, 0)      # the high word of the problem number is part of the counter


def test_the_sequential_rule_on_hand_made_cases():
  """near_tries: the 17th feasible-but-near candidate is the first one the second rule accepts; caps return the last candidate drawn."""
  H = W = 16
  f = PCS.fields(H, W)
  P = PCS.params()
  s, g, d, info = PO.sample_one(f[PCS.POCKET], P, 7, 3)
  assert info == 4
  feas = [k for k in range(d[1] + 1) if PO.is_feasible(f[PCS.POCKET], *PO.candidate(P, 7, 3, k, 1), P.clearance)]
  assert len(feas) == 17 and feas[-1] == d[1] and g == PO.candidate(P, 7, 3, d[1], 1)
  s, g, d, info = PO.sample_one(f[PCS.BLOCKED], P, 7, 3)
  assert info == 3 and d == (P.max_draws - 1, P.max_draws - 1) and s == PO.candidate(P, 7, 3, P.max_draws - 1, 0) and g == PO.candidate(P, 7, 3, P.max_draws - 1, 1)
  assert PO.sample_one(f[PCS.EMPTY], P, 7, 3, 2) == ((4.0, -4.0), (-4.0, 4.0), (-1, -1), 0)
  assert PO.sample_one(f[PCS.CORNERS], P, 7, 3, 2)[3] & 8
  few = PO.Params(PCS.CLEARANCE, max_draws=1)
  assert PO.sample_one(f[PCS.EMPTY], few, 7, 3)[2] == (0, 0)


@pytest.mark.parametrize('n', sorted(PCS.SIZES))
def test_gpu_test_inputs_take_every_branch(n):
  H, W = PCS.SIZES[n]
  f, env, diag, (start, goal, draws, info) = PCS.mixed(H, W)
  PCS.check_branches(PCS.branch_counts(env, diag, draws, info))
  per_wave = np.array([len(set(env[b:b + 4])) for b in range(0, len(env) - 3, 4)])
  assert per_wave.min() == 4      # the four lane groups of every wavefront sample four different environments
  _, _, sdiag, (_, _, sdraws, sinfo) = PCS.shared(H, W)
  assert ((sinfo & 8) != 0).sum() > 0 and (sdiag < 0).sum() > 0


# ---- the entry point, without a GPU -------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def api():
  if not os.path.exists(_capi.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _capi.get_api()


def _cfg(**kw):
  base = dict(num_states=16, dof=2, io_dtype=_capi.DGP_F64, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)
  base.update(kw)
  return _capi.make_config(**base)


def test_struct_layout_and_symbol(api):
  assert C.sizeof(_capi.DgpSampleParams) == 3 * 8 + 2 * 4 + 8      # include/dgpmp2_hip.h: three doubles, two int32, one double
  assert _capi.DgpSampleParams.corner_inset.offset == 32
  assert 'sample_problems' in _capi.CApi.SYMBOLS and api.sample_problems is not None


def test_sample_problems_validates_arguments_without_gpu(api):
  s = _capi.Solver(_cfg())
  ok_sdf, ok = s.sdf_arg(0x1000, 16, 16, 0), s.sample_params(0.9)
  call = lambda solver, sdf, p, batch=8, **kw: solver.sample_problems(batch, sdf, p, 0x1000, 0x1000, 0x1000, **kw)

  def refused(*a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      call(*a, **kw)
    return e.value
  s3 = _capi.Solver(_cfg(dof=3, Q_c_inv=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]))
  e = refused(s3, ok_sdf, ok)
  assert e.code == _capi.DGP_EINVAL and 'dof' in str(e)
  assert refused(s, ok_sdf, None).code == _capi.DGP_EINVAL                                   # NULL params
  assert refused(s, None, ok).code == _capi.DGP_EINVAL                                       # NULL sdf
  assert refused(s, s.sdf_arg(None, 16, 16, 0), ok).code == _capi.DGP_EINVAL                 # ... or no grid in it
  e = refused(s, ok_sdf, s.sample_params(0.9, max_draws=0))
  assert e.code == _capi.DGP_EINVAL and 'max_draws' in str(e)
  e = refused(s, ok_sdf, s.sample_params(0.9, margin=5.0))                                   # the box [-5 + 5, 5 - 5] is empty
  assert e.code == _capi.DGP_EINVAL and 'margin' in str(e)
  assert refused(s, ok_sdf, s.sample_params(0.9, margin=6.0)).code == _capi.DGP_EINVAL
  assert refused(s, ok_sdf, ok, batch=0).code == _capi.DGP_EINVAL
  assert api.sample_problems(None, 8, C.byref(ok_sdf), None, C.byref(ok), 0, 0, None, 0x1000, 0x1000, 0x1000, None, None, None) == _capi.DGP_EINVAL      # handle
  assert api.sample_problems(s.handle, 8, C.byref(ok_sdf), None, C.byref(ok), 0, 0, None, None, 0x1000, 0x1000, None, None, None) == _capi.DGP_EINVAL    # start


def test_front_end_refuses_host_tensors():
  import torch
  from dgpmp2_amd.datasets import problem_generation as PG
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.sample_problems(object(), torch.zeros(1, 1, 16, 16))
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.generate_dataset('unused', 'train', torch.zeros(2, 16, 16), None, 1)
