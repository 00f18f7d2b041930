"""CPU-only checks of the kernel logic: the per-lane program the HIP kernel runs (dgpmp2_amd/csrc/gn_lane.h) is
compiled for the host and executed by tests/emul's 64-thread wavefront emulator, through the same C-ABI
marshalling as the product, and compared with the oracle and the reference's golden fixtures."""
import pytest
import harness
import parity_cases as PC


@pytest.fixture(scope='module')
def be():
  return harness.Backend('emul')


# the emulator runs every lane as a thread: keep the slow cases trimmed
def test_emul_c2mini_static(be, golden): PC.case_c2mini_static(be, golden, 'f64', steps=(0, 9), nb=2)
def test_emul_c2mini_static_f32(be, golden): PC.case_c2mini_static(be, golden, 'f32', steps=(4,), nb=2)
def test_emul_c2mini_covs(be, golden): PC.case_c2mini_covs(be, golden, 'f64', nb=2)
def test_emul_per_sample_sdf(be, golden): PC.case_c2mini_per_sample_sdf(be, golden, 'f64', nb=3)
def test_emul_c1(be, golden): PC.case_c1(be, golden, 'f64', steps=(0, 9))
def test_emul_small_ragged(be, golden): PC.case_small_ragged(be, golden, 'f64')
def test_emul_small_ragged_f32(be, golden): PC.case_small_ragged(be, golden, 'f32')
def test_emul_edges(be, golden): PC.case_edges(be, golden, 'f64')
def test_emul_c3_vel(be, golden): PC.case_c3_vel(be, golden, 'f64')
def test_emul_c4_xyh(be, golden): PC.case_c4_xyh(be, golden, 'f64')
def test_emul_eval_errors(be, golden): PC.case_eval_errors(be, golden, 'f64')
def test_emul_solve(be, golden): PC.case_solve(be, golden, 'f64')
def test_emul_not_spd(be, golden): PC.case_not_spd(be, golden, 'f64')
def test_emul_backward_golden(be, golden): PC.case_backward_golden(be, golden, 'f64')
def test_emul_backward_golden_f32(be, golden): PC.case_backward_golden(be, golden, 'f32')
def test_emul_backward_fd(be, golden): PC.case_backward_fd(be, golden, 'f64')
def test_emul_tiny_sizes(be, golden): PC.case_tiny_and_odd_sizes(be, golden, 'f64')
def test_emul_sdf_grad_copies(be, golden): PC.case_shared_sdf_gradient_partial_copies(be, golden, 'f64')
def test_emul_static_qc_variants(be, golden): PC.case_static_qc_variants(be, golden, 'f64')
def test_emul_scalar_covariances(be, golden): PC.case_scalar_covariances(be, golden, 'f64')
def test_emul_scalar_covariances_f32(be, golden): PC.case_scalar_covariances(be, golden, 'f32')
def test_emul_unaligned(be, golden): PC.case_unaligned_buffers(be, golden, 'f64')
def test_emul_unaligned_f32(be, golden): PC.case_unaligned_buffers(be, golden, 'f32')
def test_emul_solve_with_covariances(be, golden): PC.case_solve_with_covariances(be, golden, 'f64')
def test_emul_eval_errors_backward(be, golden): PC.case_eval_errors_backward(be, golden, 'f64')
def test_emul_eval_errors_backward_f32(be, golden): PC.case_eval_errors_backward(be, golden, 'f32')
def test_emul_solve_backward(be, golden): PC.case_solve_backward(be, golden, 'f64')
def test_emul_solve_backward_f32(be, golden): PC.case_solve_backward(be, golden, 'f32')
def test_emul_solve_backward_general_qc(be, golden): PC.case_solve_backward_general_qc(be, golden, 'f64')
def test_emul_step_errors(be, golden): PC.case_step_errors(be, golden, 'f64')
def test_emul_step_errors_f32(be, golden): PC.case_step_errors(be, golden, 'f32')
def test_emul_sdf_gradient_delivery(be, golden): PC.case_sdf_gradient_delivery(be, golden, 'f64')
def test_emul_sdf_gradient_delivery_f32(be, golden): PC.case_sdf_gradient_delivery(be, golden, 'f32')
def test_emul_tiled_grids(golden):
  """DgpSdf::layout = DGP_SDF_TILED4 (round 5): parity cases re-run with every grid stored as 4 x 4 tiles and the dense grid gradients untiled -- per-sample and
  shared grids, non-square / odd-sized grids (padding cells), trajectories leaving the grid, the backward pass with partial copies and the training iteration."""
  bt = harness.Backend('emul'); bt.sdf_tiled = True
  PC.case_c2mini_per_sample_sdf(bt, golden, 'f64', nb=3)
  PC.case_edges(bt, golden, 'f64')
  PC.case_c1(bt, golden, 'f64', steps=(0,))
  PC.case_backward_golden(bt, golden, 'f64')
  PC.case_backward_golden(bt, golden, 'f32')
  PC.case_shared_sdf_gradient_partial_copies(bt, golden, 'f64')
  PC.case_sdf_gradient_delivery(bt, golden, 'f32')
  PC.case_step_errors(bt, golden, 'f64')
def test_emul_raw_squared_covariances(be, golden): PC.case_raw_squared_covariances(be, golden, 'f64')
def test_emul_raw_squared_covariances_f32(be, golden): PC.case_raw_squared_covariances(be, golden, 'f32')



# away from the default configuration constants (parity_cases.ND), trimmed: the rows of the forced shapes (16,4) with n = 64 and n = 13 and (16,1) with n = 13, two
# trajectories, fp64 -- the step, the fused loop, the errors, every backward against the C and the autograd oracles -- then the reference's own rows of g11; one fp32 row
_ND_EMUL = [i for i, r in enumerate(PC.ND_ROWS) if (r[2], r[3]) in (('16,4', 64), ('16,4', 13), ('16,1', 13))]


@pytest.mark.parametrize('i', _ND_EMUL, ids=lambda i: '%s-%s-n%d' % (PC.ND_ROWS[i][0].replace(' ', '_'), PC.ND_ROWS[i][2].replace(',', 'x'), PC.ND_ROWS[i][3]))
def test_emul_config_constants(be, golden, i): PC.case_config_constants(be, golden, 'f64', rows=[PC.ND_ROWS[i]], long=False, fixture=False, nb=2)
def test_emul_config_constants_fixture_rows(be, golden): PC.case_config_constants(be, golden, 'f64', rows=[], long=False)
def test_emul_config_constants_f32(be, golden): PC.case_config_constants(be, golden, 'f32', rows=[PC.ND_ROWS[2]], dofs=(2,), long=False, nb=2)


# ---- launch shapes: LPT lanes per trajectory x C states per lane (local block elimination + PCR over the lanes)
import os
import numpy as np
from conftest import rel_err
from oracle import gpmp2_oracle as O


@pytest.fixture
def force_shape():
  def setter(shape):
    if shape is None: os.environ.pop('DGP_FORCE_SHAPE', None)
    else: os.environ['DGP_FORCE_SHAPE'] = shape
  yield setter
  os.environ.pop('DGP_FORCE_SHAPE', None)


@pytest.mark.parametrize('shape', ['64,1', '32,2', '16,4', '64,2', '32,4', '64,4'])
def test_emul_shapes_n64(be, golden, force_shape, shape):
  force_shape(shape)
  g = golden('g3_c2mini')
  p = PC.P2d(64)
  sdf = O.circles_sdf(int(g['G']), g['circles'])[None, None]
  PC.check_step(be, p, g['th_hist'][3][:2], g['start'][:2], g['goal'][:2], sdf, 'f64',
                ref=(g['dth_hist'][3][:2], g['err_hist'][3][:2], g['errext_hist'][3][:2]), tag='shape ' + shape)


@pytest.mark.parametrize('shape', ['64,2', '32,4', '64,4', None])
def test_emul_n101_reference_default_length(be, golden, force_shape, shape):
  """n = 101 = the reference YAML's total_time_step=100 (examples/configs/gpmp2_2d_params.yaml:6): more states than lanes."""
  force_shape(shape)
  g = golden('g3_c1')
  p = O.OracleParams(dof=2, total_time_step=100)
  th0 = O.straight_line_trajb(g['start'][:, :, :2], g['goal'][:, :, :2], 10.0, 100, 2)
  dth, err, eex, info = be.step(p, th0, g['start'], g['goal'], g['sdf'][None, None], io='f64')
  assert rel_err(dth, g['n101_dth0']) < 1e-9 and rel_err(err, g['n101_err0'].reshape(-1)) < 1e-11 and info[0] == 0
  assert abs(float(err[0]) - 330.436499542839) < 1e-8          # survey known-answer


def test_emul_shapes_xyh_and_solve(be, golden, force_shape):
  force_shape('16,2')
  PC.case_c4_xyh(be, golden, 'f64')
  PC.case_c3_vel(be, golden, 'f64')
  force_shape('16,4')
  PC.case_solve(be, golden, 'f64')
  PC.case_eval_errors(be, golden, 'f64')


def test_force_shape_rejects_unsupported(force_shape):
  from dgpmp2_amd import _capi
  force_shape('16,2')          # 32 rows < n = 64
  with pytest.raises(_capi.DgpError):
    _capi.Solver(harness.config_from_oracle(PC.P2d(64), 'f64'), api=harness.emul_api())


@pytest.mark.parametrize('shape', ['16,2', '16,4', '32,2'])
def test_emul_backward_shapes(be, golden, force_shape, shape):
  force_shape(shape)
  PC.case_backward_golden(be, golden, 'f64')


@pytest.mark.parametrize('n', [64, 63])
def test_emul_chain_backward_woodbury_exact_and_ragged(be, force_shape, n):
  """dgp_gn_solve_backward on the forced shape (16,4): n = 64 fills it (the QK_WB chain kernel), n = 63 does not (QK_WBR).  f64, B = 2, K = 2, against the
  single-step backward launches chained by hand through the traced history (lane_mix.chain_walk), at lane_mix's bound for the static Woodbury chain.
  The emulator must run the chain program the product launches here: before the kernel selection was shared, its own dispatch ran the single-step
  backward program at n = 64, which reads the null dtheta of a chain call: the n = 64 case ended in a segmentation fault inside emul_gn_solve_backward."""
  import lane_mix as LM
  from dgpmp2_amd import _capi
  force_shape('16,4')
  bt = LM.make(2, 16, 4, n, 'static', waves=0, nan=False, io='f64', seed=n)
  assert bt.B == 2
  assert _capi.Solver(harness.config_from_oracle(bt.p, 'f64'), api=be.api).step_kernel_variant(bt.B) == LM.expected_variant(16, 4, n, 'static', False) == (3 if n == 64 else 4)
  K = 2
  tho, its, hist = be.solve_traced(bt.p, bt.th, bt.start, bt.goal, bt.sdf, K, 0.0, io='f64')[:3]
  assert (its == K).all()
  gbar = np.random.RandomState(7).randn(bt.B, n, 4)
  got = be.solve_backward(bt.p, bt.start, bt.goal, bt.sdf, K, hist, tho, its, gbar, io='f64')
  want = LM.chain_walk(be, bt, K, hist, tho, its, gbar, 'f64', 'dense')
  bad = LM.check_grads(bt, 'chain backward vs chained steps', got, want, LM.CHAIN_TOL['static'], LM.ok_rows(bt), keys=('th', 'start', 'goal'))
  assert not bad, '\n'.join(bad)


def test_emul_woodbury_kernels(be, golden):
  """gn_woodbury.h on the emulator: the smallest shape in full, the two larger ones with one robot each (64 threads per wavefront)."""
  PC.case_woodbury_kernels(be, golden, 'f64', shapes=('16,4',), nb=2)


def test_emul_woodbury_kernels_f32_and_wide_shapes(be, golden):
  PC.case_woodbury_kernels(be, golden, 'f32', shapes=('32,4',), nb=1)


def test_emul_long_trajectories(be, golden):
  """n > 256 through the loop kernels of gn_long.h (see parity_cases.case_long_trajectories), trimmed for the thread-per-lane emulator."""
  PC.case_long_trajectories(be, golden, 'f64', configs=[(2, 300, 'perstate', dict(use_vel_limits=True, K_v=0.01, v_x=0.5, v_y=0.5)),
                                                        (3, 257, 'static', dict(non_holonomic=True, K_d=0.05)), (3, 320, 'qfull', {})])


def test_emul_long_trajectories_f32(be, golden):
  PC.case_long_trajectories(be, golden, 'f32', configs=[(2, 300, 'static', {})])


# ---- call forms (tests/call_forms.py): optional pointers NULL and buffers off the 16-byte boundary must not change a result -- the GPU test's case trimmed to three
# trajectories on twelve (configuration, entry-point group) pairs: the forced shapes (16,4) exact and ragged, (16,2) at d = 6 and (64,1); static, per-state and scalar
# covariances; both I/O types; one n = 257.  The SOURCE satisfies the invariants exactly (this test); whether every compiled instantiation does is test_hip_call_forms.py's.
import call_forms as CF

_CF_EMUL = [
  (CF.Cfg(2, 'f64', (16, 4), 64, 'static', grid='per', B=3), ('forward', 'backward')),
  (CF.Cfg(2, 'f64', (16, 4), 64, 'static', grid='shared16', B=3), ('errs',)),
  (CF.Cfg(2, 'f64', (16, 4), 61, 'static', grid='shared1', B=3), ('loop',)),
  (CF.Cfg(2, 'f32', (16, 4), 61, 'perstate', grid='per', B=3), ('backward',)),
  (CF.Cfg(2, 'f32', (16, 4), 64, 'scalar', grid='shared1', B=3), ('forward', 'errs')),
  (CF.Cfg(3, 'f64', (16, 2), 29, 'static', grid='per', B=3), ('loop',)),
  (CF.Cfg(3, 'f32', (16, 2), 29, 'perstate', grid='shared16', B=3), ('backward',)),
  (CF.Cfg(3, 'f64', (16, 2), 29, 'scalar', grid='shared1', B=3), ('errs',)),
  (CF.Cfg(2, 'f64', (64, 1), 64, 'perstate', grid='shared1', B=3), ('backward',)),
  (CF.Cfg(2, 'f32', (64, 1), 64, 'static', grid='per', B=3), ('forward',)),
  (CF.Cfg(3, 'f32', (16, 4), 64, 'static', grid='shared1', B=3), ('errs',)),
  (CF.long_configs('f64')[0], ('forward', 'backward')),
]


@pytest.mark.parametrize('i', range(len(_CF_EMUL)), ids=lambda i: ('%s-%s' % (_CF_EMUL[i][0].tag(), '+'.join(_CF_EMUL[i][1]))).replace(' ', '_'))
def test_emul_call_forms(i):
  c, groups = _CF_EMUL[i]
  b = harness.Backend('emul')
  fails = []
  compared = CF.run_config(b, c, groups, fails)
  assert b.guard_checks > 0 and b.input_checks > 0 and compared > 0
  assert not fails, '%d call forms differ from the canonical call:\n' % len(fails) + '\n'.join(map(str, fails[:40]))


# ---- the per-trajectory SPD flag `info` against an inertia reference (tests/spd_cases.py): the CPU-only conditions on the inputs and the two references, then a
# trimmed selection of tests/test_hip_spd_flag.py through the emulator (every lane a thread: n <= 64)
import lane_mix as LM
import spd_cases as SC

_NT = max(1, min(16, os.cpu_count() or 1))


@pytest.mark.parametrize('dof', [2, 3])
def test_spd_references_and_conditions(dof):
  """Oracle alone, every configuration tests/test_hip_spd_flag.py runs: at most 10 % of the trajectories of a (configuration, rung) undecided or excluded by the
  loop's chain; a rung with a decided-clean and a decided-flagged trajectory in one wavefront (shapes with two or more trajectories per wavefront); and for
  n d <= 256 the dense numpy oracle -- eigvalsh(LAM).min() <= 0 -- agrees with the long-double C oracle on every decided trajectory at every rung, and
  spd_cases.diag_lam (the scale of delta at any n) is the dense LAM's diagonal."""
  bad = []
  compared = 0
  for cfg, grid, seed in SC.all_configs(dof):
    bt = SC.batch(dof, cfg, grid, seed)
    refs = SC.references(bt, _NT)
    bad += SC.check_conditions(bt, refs)
    if bt.n * 2 * dof > 256: continue
    for reg, (r, _, _) in refs.items():
      lam = SC.dense_lam(bt, bt.th, reg)
      dg = np.einsum('bii->bi', lam)
      if not np.allclose(SC.diag_lam(bt, bt.th, reg), dg, rtol=1e-12, atol=1e-12 * np.abs(dg).max()): bad.append('%s reg %g: diag_lam differs from the dense diagonal' % (bt.tag, reg))
      dense = (np.linalg.eigvalsh(lam).min(1) <= 0).astype(np.int32)
      bad += SC._flag_fails(bt, 'reg %g dense oracle' % reg, dense, r.verdict, r.decided)
      compared += int(r.decided.sum())
  assert compared > 1000
  assert not bad, '\n'.join(bad)


# one shape per LPT ((16,4), (32,2), (64,1)) and each covariance family at d = 4 -- the families spread over the three shapes --, and one d = 6 Woodbury
# configuration; every one runs the fused loop (and the traced loop where static) on spd_cases.trimmed_rungs
_SPD_SHAPES = ((16, 4), (32, 2), (64, 1))
_SPD_EMUL = [(2, (16, 4, 64, 'static', False)), (2, (16, 4, 61, 'qfull', False)), (2, (32, 2, 61, 'static_full', False)), (2, (32, 2, 64, 'perstate', False)),
             (2, (32, 2, 61, 'scalar', False)), (2, (64, 1, 64, 'static_diag', True)), (2, (64, 1, 64, 'perstate', True)), (3, (16, 4, 64, 'static', False))]


def test_spd_emulator_selection():
  covs = set(cf[3].split('_raw')[0] for d, cf in _SPD_EMUL if d == 2)
  assert covs >= {'static', 'static_full', 'static_diag', 'perstate', 'qfull', 'scalar'} and set(cf[:2] for _, cf in _SPD_EMUL) == set(_SPD_SHAPES), _SPD_EMUL
  assert all(cf in LM.configs(d) for d, cf in _SPD_EMUL)      # (the GPU test's own configurations, seeded alike)
  assert all(cf[2] <= 64 for _, cf in _SPD_EMUL) and any(d == 3 and LM.expected_variant(*cf) in (3, 4) for d, cf in _SPD_EMUL)


@pytest.mark.parametrize('dof,cfg', _SPD_EMUL, ids=lambda v: v if isinstance(v, int) else '%d_%d_n%d_%s' % v[:4])
def test_emul_spd_flag(dof, cfg, monkeypatch):
  """tests/test_hip_spd_flag.py on the emulator: lever A on three rungs (f64; one configuration of each shape on the mixed rung in f32 as well), lever B where the mode has
  per-call covariance tensors"""
  monkeypatch.setenv('DGP_FORCE_SHAPE', '%d,%d' % cfg[:2])
  bt = SC.batch(dof, cfg, None, 1000 * dof + 10 * cfg[0] + cfg[1])
  be = harness.Backend('emul')
  only = SC.trimmed_rungs(bt, SC.references(bt, _NT))
  bad = SC.run_ladder(be, bt, 'f64', nthreads=_NT, only=only)
  if cfg[3] in ('qfull', 'static_full', 'static_diag'): bad += SC.run_ladder(be, bt, 'f32', nthreads=_NT, alone=False, rotation=False, only=only[1:2])
  if cfg[3] in SC.LEVER_B_COVS: bad += SC.run_lever_b(be, bt, 'f64', nthreads=_NT)
  assert not bad, '%d failures:\n' % len(bad) + '\n'.join(bad[:40])
