"""dgp_sdf_lookup / dgp_sdf_lookup_backward on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through Python.

  * forward against tests/lookup_oracle.py: d_obs, J and the five summary columns bit for bit, fp64 and fp32 (fp32: the oracle on the fp32-valued inputs, cast once),
    with a clearance that ties in the middle row (the `<=`);
  * backward: g_points bit for bit; the grid gradient bit for bit in every cell that receives at most one contribution (whole grids in the disjoint cases), within
    (K + 1) u sum|t_i| in a cell with K contributions, u = 2^-53 for fp64 accumulators (fp64 I/O, DGP_GSDF_DENSE_F64) and 2^-24 for fp32 ones;
  * shapes: B in {1, 3, 5} x S in {1, 3, 16, 17, 33, 65, 130} (all three lanes-per-row instantiations, asserted; ragged last wavefronts), shared, per-sample and
    tiled grids, point_stride 2 and 4, the four frames of tests/lookup_cases.py (5 x 7, 2 x 2 and 40 x 32 grids; points on cell lines, in clamped cells, at +-1e6);
  * call forms under guard bands: every optional pointer NULL in turn, every buffer off the 16-byte boundary -- the canonical call's bits;
  * through Python: bilinear_interpolate on device tensors against the CPU mirror, loss.backward() through both outputs, a th[:, :, :2] view read in place,
    check_solved[_batch] on the reference's fixture, planner.check_solved against trajectory_metrics' in_collision."""
import numpy as np
import pytest
import torch

import harness
import lookup_cases as LC
import lookup_oracle as LO
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BS, SS = (1, 3, 5), (1, 3, 16, 17, 33, 65, 130)
FRAME_ORDER = ('g1', '5x7', '2x2', 'g1_cell')
KINDS = ('shared', 'per_sample', 'tiled')      # tiled: per-sample for odd B, shared for even positions (both occur)


@pytest.fixture(scope='module')
def be():
  b = harness.Backend('hip')
  yield b
  b.guard = b.misalign = False


def _code(io): return _capi.DGP_F64 if io == 'f64' else _capi.DGP_F32


def _grid_dev(be, grid, io, tiled, name='sdf'):
  """grid (G, H, W) -> (DgpSdf fields without the gradient mode, elements per grid)"""
  G, H, W = grid.shape
  flat = LC.tile(grid) if tiled else grid.reshape(G, -1)
  _, ptr = be.to_dev(flat, io, name=name)
  return (ptr, H, W, 0 if G == 1 else flat.shape[1], _capi.DGP_SDF_TILED4 if tiled else _capi.DGP_SDF_ROWMAJOR), flat.shape[1]


def _wide_points(pts, stride, seed=3):
  if stride == 2: return pts
  out = np.random.RandomState(seed).uniform(-9, 9, pts.shape[:2] + (stride,))
  out[:, :, :2] = pts
  return out


def fwd(be, grid, pts, frame, io, tiled=False, stride=2, clearance=0.0, want=('d', 'J', 's')):
  """dgp_sdf_lookup -> {'d': (B,S), 'J': (B,S,2), 's': (B,5)} (None for an output left out)"""
  be._keep, be._rec = [], {}
  B, S, _ = pts.shape
  res = LC.FRAMES[frame][1]
  sd, _ = _grid_dev(be, grid, io, tiled)
  _, p = be.to_dev(_wide_points(pts, stride), io, name='points')
  d = be.empty((B, S), io, name='d_obs') if 'd' in want else (None, None)
  J = be.empty((B, S, 2), io, name='J') if 'J' in want else (None, None)
  s = be.empty((B, _capi.DGP_LOOKUP_COUNT), dtype=np.float64, name='summary') if 's' in want else (None, None)
  _capi.sdf_lookup(_code(io), B, S, p, stride, _capi.Solver.sdf_arg(*sd), res, LC.X_LIMS, LC.Y_LIMS, clearance, d[1], J[1], s[1], stream=be.stream())
  out = {'d': be.to_np(d[0]), 'J': be.to_np(J[0]), 's': be.to_np(s[0])}
  be._done()
  return out


def bwd(be, grid, pts, frame, io, g_d, g_J, tiled=False, stride=2, wide=False, want=('p', 'g')):
  """dgp_sdf_lookup_backward -> {'p': g_points (B,S,2), 'g': the grid gradient (G,H,W), untiled}"""
  be._keep, be._rec = [], {}
  B, S, _ = pts.shape
  G, H, W = grid.shape
  res = LC.FRAMES[frame][1]
  sd, elems = _grid_dev(be, grid, io, tiled)
  _, p = be.to_dev(_wide_points(pts, stride), io, name='points')
  _, gd = be.to_dev(g_d, io, name='g_d')
  _, gj = be.to_dev(g_J, io, name='g_J')
  gp = be.empty((B, S, 2), io, name='g_points') if 'p' in want else (None, None)
  acc = np.float64 if (wide or io == 'f64') else np.float32
  gs = be.empty((G, elems), dtype=acc, fill=0.0, name='g_sdf') if 'g' in want else (None, None)
  mode = _capi.DGP_GSDF_DENSE_F64 if wide else _capi.DGP_GSDF_DENSE
  _capi.sdf_lookup_backward(_code(io), B, S, p, stride, _capi.Solver.sdf_arg(*sd, grad_mode=mode), res, LC.X_LIMS, LC.Y_LIMS, gd, gj, gp[1], gs[1], 0 if G == 1 else elems, 1,
                            stream=be.stream())
  g = be.to_np(gs[0])
  out = {'p': be.to_np(gp[0]), 'g': None if g is None else (LC.untile(g, H, W) if tiled else g.reshape(G, H, W))}
  be._done()
  return out


def check_forward(tag, got, grid, pts, frame, io, clearance):
  d, J, s = LO.forward(grid, pts, LC.FRAMES[frame][1], LC.X_LIMS, LC.Y_LIMS, clearance, io)
  bad = []
  for k, want in (('d', d), ('J', J), ('s', s)):
    if got[k] is not None and not LC.same_bits(got[k], want):
      bad.append('%s: %s differs from the oracle in %d entries' % (tag, k, int((LC.bits(got[k]) != LC.bits(want)).sum())))
  return bad


def check_backward(tag, got, grid, pts, frame, io, g_d, g_J, wide=False):
  ref = LO.backward(grid, pts, LC.FRAMES[frame][1], LC.X_LIMS, LC.Y_LIMS, g_d, g_J, io=io, shared=grid.shape[0] == 1, wide=wide)
  bad = []
  if got['p'] is not None and not LC.same_bits(got['p'], ref['g_points']):
    bad.append('%s: g_points differs from the oracle in %d entries' % (tag, int((LC.bits(got['p']) != LC.bits(ref['g_points'])).sum())))
  if got['g'] is not None:
    u = LO.U64 if (wide or io == 'f64') else LO.U32
    bound = LO.grid_bound(ref, u)
    err = np.abs(got['g'] - ref['g_sdf'])
    single = ref['count'] <= 1
    if not LC.same_bits(got['g'][single], ref['g_sdf'][single]): bad.append('%s: a cell of the grid gradient with at most one contribution is not that contribution' % tag)
    if not (err <= bound).all(): bad.append('%s: the grid gradient is at %.3g of its bound' % (tag, float((err[~single] / bound[~single]).max())))
  return bad, ref


def _case(B, S, kind, i):
  frame = FRAME_ORDER[i % len(FRAME_ORDER)]
  shared = kind == 'shared' or (kind == 'tiled' and i % 2 == 0)
  grid = LC.grids(LC.FRAMES[frame][0], 1 if shared else B)
  return frame, grid, LC.points(frame, B, S, seed=i)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_every_shape_against_the_oracle(be, io, kind):
  bad, lpts, frames = [], set(), set()
  i = 0
  for B in BS:
    for S in SS:
      lpts.add(LO.lpt(S))
      for stride in (2, 4):
        i += 1
        frame, grid, pts = _case(B, S, kind, i)
        frames.add(frame)
        tiled = kind == 'tiled'
        wide = io == 'f32' and grid.shape[0] == 1 and i % 4 < 2      # fp32 I/O on a shared grid: fp64 accumulators in half of the cases
        clearance = float(LO.distance(grid, pts, LC.FRAMES[frame][1], LC.X_LIMS, LC.Y_LIMS, io)[B // 2].min())
        tag = '%s %s B %d S %d stride %d %s' % (io, kind, B, S, stride, frame)
        bad += check_forward(tag, fwd(be, grid, pts, frame, io, tiled, stride, clearance), grid, pts, frame, io, clearance)
        g_d, g_J = LC.cotangents(B, S, seed=i)
        bad += check_backward(tag, bwd(be, grid, pts, frame, io, g_d, g_J, tiled, stride, wide), grid, pts, frame, io, g_d, g_J, wide)[0]
  assert lpts == {16, 32, 64} and frames == set(FRAME_ORDER)
  assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_disjoint_footprints_give_the_oracle_grid_bit_for_bit(be, io):
  """every cell receives at most one contribution: the atomics add to zero once, the whole grid gradient has the oracle's bits"""
  ran = 0
  for B, S, shared, tiled in ((3, 33, True, False), (5, 17, True, True), (3, 65, False, False), (5, 130, False, True), (1, 130, True, False)):
    pts = LC.disjoint_points('g1', B, S, shared, seed=S)
    assert pts is not None
    grid = LC.grids('g1', 1 if shared else B)
    g_d, g_J = LC.cotangents(B, S, seed=2)
    for wide in ((False, True) if io == 'f32' else (False,)):
      got = bwd(be, grid, pts, 'g1', io, g_d, g_J, tiled, 2, wide)
      bad, ref = check_backward('disjoint %s B %d S %d' % (io, B, S), got, grid, pts, 'g1', io, g_d, g_J, wide)
      assert ref['count'].max() == 1 and ref['count'].sum() == 4 * B * S and not bad, bad
      assert LC.same_bits(got['g'], ref['g_sdf'])
      ran += 1
  assert ran >= 5


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_call_forms_reproduce_the_canonical_call(be, io):
  """every optional pointer NULL in turn and every buffer off the 16-byte boundary, under guard bands (no store outside an output, no store into an input): the bits
  of the canonical call.  The grid gradient is compared where it is deterministic (disjoint footprints) and held to the oracle's bound in the mixed case."""
  for B, S, stride, tiled, disjoint in ((3, 33, 2, False, True), (5, 17, 4, True, False), (3, 65, 2, True, True), (1, 130, 2, False, False)):
    frame = 'g1'
    grid = LC.grids('g1', B)
    pts = LC.disjoint_points(frame, B, S, False, seed=1) if disjoint else LC.points(frame, B, S, seed=5)
    g_d, g_J = LC.cotangents(B, S, seed=4)
    clearance = float(LO.distance(grid, pts, LC.FRAMES[frame][1], LC.X_LIMS, LC.Y_LIMS, io)[B // 2].min())
    ref_f = fwd(be, grid, pts, frame, io, tiled, stride, clearance)
    ref_b = bwd(be, grid, pts, frame, io, g_d, g_J, tiled, stride)
    assert not check_forward('canonical', ref_f, grid, pts, frame, io, clearance) and not check_backward('canonical', ref_b, grid, pts, frame, io, g_d, g_J)[0]
    zero = np.zeros_like
    be.guard = True
    try:
      checks = be.guard_checks
      for mis in (False, True, 'inputs', 'outputs'):
        be.misalign = mis
        tag = (io, B, S, stride, tiled, mis)
        for want in (('d', 'J', 's'), ('d',), ('J',), ('s',), ('d', 's'), ('J', 's')):
          got = fwd(be, grid, pts, frame, io, tiled, stride, clearance, want=want)
          assert all((got[k] is None) == (k not in want) for k in 'dJs') and all(LC.same_bits(got[k], ref_f[k]) for k in want), (tag, want)
        for want in (('p', 'g'), ('p',), ('g',)):
          got = bwd(be, grid, pts, frame, io, g_d, g_J, tiled, stride, want=want)
          if 'p' in want: assert LC.same_bits(got['p'], ref_b['p']), (tag, want)
          if 'g' in want:
            if disjoint: assert LC.same_bits(got['g'], ref_b['g']), (tag, want)
            else: assert not check_backward(str(tag), dict(got, p=None), grid, pts, frame, io, g_d, g_J)[0]
      be.misalign = False
      # a NULL cotangent is a zero cotangent
      for gd_, gj_ in ((None, g_J), (g_d, None)):
        got = bwd(be, grid, pts, frame, io, gd_, gj_, tiled, stride)
        zeroed = bwd(be, grid, pts, frame, io, zero(g_d) if gd_ is None else g_d, zero(g_J) if gj_ is None else g_J, tiled, stride)
        assert LC.same_bits(got['p'], zeroed['p']) and not check_backward('null cotangent', got, grid, pts, frame, io, gd_, gj_)[0]
        if disjoint: assert LC.same_bits(got['g'], zeroed['g'])
      assert be.guard_checks > checks + 4 * 9
    finally:
      be.guard = be.misalign = False


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_rows_do_not_depend_on_batch_position_and_nan_is_contained(be, io):
  B, S, frame = 5, 65, '5x7'
  grid, pts = LC.grids('5x7', B), LC.points('5x7', B, S, seed=9)
  ref = fwd(be, grid, pts, frame, io, clearance=0.25)
  rolled = fwd(be, np.roll(grid, 1, 0), np.roll(pts, 1, 0), frame, io, clearance=0.25)
  assert all(LC.same_bits(rolled[k], np.roll(ref[k], 1, 0)) for k in 'dJs')
  head = fwd(be, grid[:3], pts[:3], frame, io, clearance=0.25)
  assert all(LC.same_bits(head[k], ref[k][:3]) for k in 'dJs')
  # a NaN coordinate: that point's outputs are NaN, it wins the row's minimum, does not block, and touches nothing else
  pts2 = pts.copy()
  pts2[2, 40, 0] = np.nan
  got = fwd(be, grid, pts2, frame, io, clearance=0.25)
  assert not check_forward('nan', got, grid, pts2, frame, io, 0.25)
  assert np.isnan(got['d'][2, 40]) and np.isnan(got['d']).sum() == 1 and np.isnan(got['s'][2, 3]) and got['s'][2, 4] == 40 and not np.isnan(np.delete(got['s'], 2, 0)).any()
  assert got['s'][2, 1] == ref['s'][2, 1] - (1 if ref['d'][2, 40] <= 0.25 else 0)


def _t(a, dtype): return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class _Recorder(object):
  """the trampoline with the addresses of its sdf_lookup calls written down"""
  def __init__(self, pc): self.pc, self.points = pc, []

  def __getattr__(self, name): return getattr(self.pc, name)

  def sdf_lookup(self, *a):
    self.points.append((a[3], a[4]))
    return self.pc.sdf_lookup(*a)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_bilinear_interpolate_on_device_against_the_cpu_mirror(dtype, monkeypatch):
  from dgpmp2_amd.utils import sdf_utils as SU
  io = 'f64' if dtype is torch.float64 else 'f32'
  for frame, B, S, form in (('g1', 5, 17, 'per_sample'), ('g1_cell', 3, 65, 'shared'), ('5x7', 3, 33, 'tiled'), ('2x2', 1, 130, '3d')):
    res = LC.FRAMES[frame][1]
    shared = form == 'shared'
    grid = LC.as_io(LC.grids(LC.FRAMES[frame][0], 1 if shared else B), io)
    pts = LC.as_io(LC.points(frame, B, S, seed=3), io)
    g_d, g_J = LC.cotangents(B, S, seed=6)

    def run(dev):
      base = torch.from_numpy(grid).to(dtype).to(dev).unsqueeze(1).requires_grad_(True)      # (G,1,H,W) leaf
      im = base.expand(B, -1, -1, -1) if shared else base
      if form == 'tiled': im = SU.tile_sdf(base)
      if form == '3d': im = base[:, 0]
      st = torch.from_numpy(pts).to(dtype).to(dev).requires_grad_(True)
      d, J = SU.bilinear_interpolate(im, st, res, LC.X_LIMS, LC.Y_LIMS, use_cuda=dev != 'cpu')
      loss = (d[:, :, 0] * torch.from_numpy(g_d).to(dtype).to(dev)).sum() + (J * torch.from_numpy(g_J).to(dtype).to(dev)).sum()
      loss.backward()
      return [t.detach().double().cpu().numpy() for t in (d, J, st.grad, base.grad)] + [d.dtype, J.dtype]
    dev_out, cpu_out = run(DEV), run('cpu')
    tag = (frame, form, io)
    assert dev_out[4] is dtype and dev_out[5] is dtype and dev_out[0].shape == (B, S, 1) and dev_out[1].shape == (B, S, 2)
    assert LC.same_bits(dev_out[0], cpu_out[0]) and LC.same_bits(dev_out[1], cpu_out[1]), tag                     # the same operations in the same order, rounded once
    ref = LO.backward(grid, pts, res, LC.X_LIMS, LC.Y_LIMS, g_d, g_J, io=io, shared=shared, wide=shared)
    assert LC.same_bits(dev_out[2], ref['g_points']), tag                                                           # the kernel's closed form
    u = LO.U64 if io == 'f64' else LO.U32
    # against the mirror's autograd (another expression tree, and for fp32 gradients rounded at every step): the rounding bound of each side, added
    assert (np.abs(dev_out[2] - cpu_out[2]) <= 2 * (LO.R_POINT + 1) * u * ref['abs_points']).all(), tag
    assert dev_out[3].shape == cpu_out[3].shape == (grid.shape[0], 1) + grid.shape[1:]
    gbound = (LO.R_TAP + ref['count'] + 1) * u * 2 * ref['abs_terms']
    assert (np.abs(dev_out[3][:, 0] - cpu_out[3][:, 0]) <= gbound).all() and np.abs(dev_out[3]).max() > 0, tag
  # a position view of a trajectory tensor is read in place; a double backward raises; a modified input is caught
  pc = _Recorder(_capi.get_pycall())
  monkeypatch.setattr(_capi, '_pycall', pc)
  th = torch.randn(4, 16, 4, dtype=dtype, device=DEV).requires_grad_(True)
  sdf = torch.from_numpy(LC.grids('g1', 1)).to(dtype).to(DEV).unsqueeze(1)
  d, J = SU.bilinear_interpolate(sdf.expand(4, -1, -1, -1), th[:, :, :2], 10.0 / 32, LC.X_LIMS, LC.Y_LIMS)
  assert pc.points[-1] == (th.data_ptr(), 4)
  want_d, want_J = SU.bilinear_interpolate_torch(sdf.cpu(), th.detach().cpu()[:, :, :2], 10.0 / 32, LC.X_LIMS, LC.Y_LIMS)
  assert torch.equal(d.cpu(), want_d) and torch.equal(J.cpu(), want_J)
  d.sum().backward()
  assert th.grad.shape == th.shape and not th.grad[:, :, 2:].any() and th.grad[:, :, :2].abs().max() > 0
  with pytest.raises(RuntimeError):
    torch.autograd.grad(torch.autograd.grad(SU.bilinear_interpolate(sdf, th[:1, :, :2], 0.3, LC.X_LIMS, LC.Y_LIMS)[0].sum(), th, create_graph=True)[0].sum(), th)
  st = torch.zeros(1, 3, 2, dtype=dtype, device=DEV, requires_grad=True).clone()
  d, _ = SU.bilinear_interpolate(sdf, st, 0.3, LC.X_LIMS, LC.Y_LIMS)
  st.add_(1.0)
  with pytest.raises(RuntimeError, match='modified by an inplace operation'):
    d.sum().backward()


def test_check_solved_on_device_gives_the_reference_verdicts(golden):
  from dgpmp2_amd.utils import learn_utils as LU
  from dgpmp2_amd.utils import sdf_utils as SU
  from test_lookup_oracle import ENV, fixture_cases
  for name, frame, res, B, S, shared, grid, ref in fixture_cases(golden('g13_sdf_lookup')):
    traj = torch.cat([_t(ref['points'], torch.float64), torch.zeros(B, S, 2, dtype=torch.float64, device=DEV)], -1)
    sdf = _t(grid, torch.float64).unsqueeze(1)
    if shared: sdf = sdf.expand(B, -1, -1, -1)
    clr = float(ref['clearance'])
    batch = LU.check_solved_batch(traj, sdf, clr, res, ENV)
    assert batch.is_cuda and batch.dtype == torch.int64 and batch.tolist() == ref['solved'].tolist(), name
    assert [LU.check_solved(traj[b:b + 1], sdf[b:b + 1], clr, res, ENV, True) for b in range(B)] == ref['solved'].tolist(), name
    r = SU.sdf_lookup(sdf, traj[:, :, :2], res, LC.X_LIMS, LC.Y_LIMS, clr)
    want = LO.forward(grid, ref['points'], res, LC.X_LIMS, LC.Y_LIMS, clr)
    assert LC.same_bits(r.raw.cpu().numpy(), want[2]) and LC.same_bits(r.d_obs.cpu().numpy()[:, :, 0], ref['d_obs'][:, :, 0]) and LC.same_bits(r.J.cpu().numpy(), ref['J'])
    assert r.solved.tolist() == [bool(v) for v in ref['solved']] and r.first_blocked.dtype == torch.int64


def _planner(n, B):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_planner_check_solved_agrees_with_trajectory_metrics(dtype):
  """where the two definitions coincide -- clearance = sphere radius + the metrics' epsilon (0), end states in free space, no exact tie -- check_solved is the
  negation of trajectory_metrics' in_collision; tiled grids give the same verdicts"""
  from dgpmp2_amd.utils import sdf_utils as SU
  from oracle import gpmp2_oracle as O
  n, B, G = 17, 33, 64
  planner = _planner(n, B)
  rs = np.random.RandomState(4)
  sdf_np = O.circles_sdf(G, O.C2_CIRCLES)
  start, goal = np.zeros((B, 1, 4)), np.zeros((B, 1, 4))
  k = 0
  while k < B:      # end states well clear of the three circles
    s, g = rs.uniform(-4.5, 4.5, 2), rs.uniform(-4.5, 4.5, 2)
    if min(np.hypot(p[0] - c[0], p[1] - c[1]) - c[2] for p in (s, g) for c in O.C2_CIRCLES) > 0.8:
      start[k, 0, :2], goal[k, 0, :2] = s, g
      k += 1
  th = _t(O.straight_line_trajb(start[:, :, :2], goal[:, :, :2], 10.0, n - 1, 2), dtype)
  sdf = _t(sdf_np, dtype)[None, None].expand(B, 1, G, G)
  solved = planner.check_solved(th, sdf)
  in_coll = planner.trajectory_metrics(th, sdf).in_collision
  assert solved.dtype == torch.bool and solved.shape == (B,) and torch.equal(solved, ~in_coll) and 0 < int(solved.sum()) < B
  look = SU.sdf_lookup(sdf, th[:, :, :2], 10.0 / G, LC.X_LIMS, LC.Y_LIMS, 0.4)
  assert torch.equal(look.solved, solved) and bool((look.d_obs[:, [0, -1], 0] > 0.4).all())      # the resolution is the padded width's; the end states are free
  assert torch.equal(planner.check_solved(th, SU.tile_sdf(sdf[:1].contiguous()).expand(B, -1, -1, -1, -1, -1)), solved)
  assert not bool(planner.check_solved(th, sdf, clearance=100.0).any()) and bool(planner.check_solved(th, sdf, clearance=-100.0).all())
