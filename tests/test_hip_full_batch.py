"""GPU (-m gpu): every kernel family on full-GPU, lane-mixed batches (tests/lane_mix.py), per trajectory.

The every-kernel tests (tests/test_hip_every_kernel.py) run each instantiation on one or two wavefronts of smooth in-grid
trajectories: no SIMD ever runs a second wavefront and the data-dependent branches take the same side in nearly every lane,
so per-lane state that goes stale at a divergent join cannot show.  Here, for 2 robots x the 9 forced launch
shapes x the 6 covariance modes (velocity limits on d = 4 in one of the first four modes per shape; exact fit and ragged lengths alternating;
'static_diag' -- block elimination with C = 4 and without Woodbury -- and 'scalar' -- DGP_QC_SCALAR, the learned mode, also through the raw
output vector -- at MIN_WAVES; lane_mix.configs) and one configuration per robot with per-sample grids of an odd size,
on >= 2048 wavefronts per launch, the fp64 and the fp32 I/O kernels are held, per trajectory, to:
  (a) the C oracle's step (dtheta; err and err_ext per trajectory at 10 x TOL_ERR; info 0 except on the NaN trajectories);
  (b) the fused loop, K = 3 with tol_delta at the median first-step norm (iteration counts differ inside the wavefronts), against
      chained C-oracle steps under the same stopping rule -- trajectories whose step norm lies within 1e-6 of tol_delta are excluded
      and counted, at most 0.5 %;
  (c) themselves on the same batch rotated by TPW // 2 + 1 trajectories, bit for bit: step, fused loop, backward, and (where the family
      exists) traced loop + chain backward, step-errors + its backward, the tiled twins, the loop kernels of gn_long.h; the shared grid's
      gradient to lane_mix.SDF_ROT_TOL = 7e-11 of max|g_th| (its float64 atomics land in another order: 6.8e-12 measured, 1e-12 cannot hold);
  (d) the fp64 siblings (fp32 I/O kernels, the same numbers) at 1e-6 per trajectory;
  (e) the f64 backward against torch autograd (oracle/autograd_torch.py) on 4-6 trajectories (lane_mix.autograd_picks: first, middle and
      ragged last wavefront, different lane offsets, a mixed-hinge one) at 1e-6, and against a central difference of the extended-precision
      C oracle on EVERY trajectory along two directions: one over th, start, goal (and qc, ow, eps in per-state modes) at lane_mix.FD_TOL,
      one over the th rows of a single lane (every lane over the batch) at lane_mix.FD_LANE_TOL, which resolves a 1e-3 error in one lane; trajectories
      whose bilinear cell, hinge or velocity-limit decisions change within +-h are excluded and counted.  The shared grid's gradient
      is left out of (e): it is a sum over the batch, held to the autograd oracle by the every-kernel tests;
  (f) NaN isolation: the wave neighbours of the NaN trajectories bit-equal to the same batch without the NaN.
The twin families are held per trajectory to references as well, not only to themselves under rotation (a twin wrong the same way wherever the
trajectory sits passes (c)): the step-errors twins against the same batch's step and unweighted_errors_batch at th + dtheta, their backward against
its two halves run by hand; dgp_eval_errors (+ backward) against the C oracle, unweighted_errors_batch, autograd and a central difference; the tiled
twins against the row-major kernels; the chain backward against the single-step backward launches walked through the traced history; the static
kernel variant each static configuration launches against lane_mix.expected_variant.
Part 3 of the same issue, test_hip_headline_ten_iterations_full_size: BASELINE configs[1..3] at B = 4096 x 64, 10 iterations (lane_mix.headline).
A failure names the kernel's configuration, the trajectory, its wavefront and its lane offset."""
import time
import pytest
import harness
import lane_mix as LM

pytestmark = pytest.mark.gpu
NTHREADS = 16      # C oracle threads


@pytest.fixture(scope='module')
def be():
  import torch
  assert torch.cuda.is_available(), 'the -m gpu tests need a GPU'
  return harness.Backend('hip')


@pytest.mark.parametrize('lpt', [16, 32, 64])
@pytest.mark.parametrize('dof', [2, 3])
def test_hip_full_batch_lane_mixed(be, dof, lpt, monkeypatch):
  bad = []
  for (l, c, n, cov, vel) in LM.configs(dof):
    if l != lpt: continue
    monkeypatch.setenv('DGP_FORCE_SHAPE', '%d,%d' % (l, c))
    t0 = time.time()
    bt = LM.make(dof, l, c, n, cov, vel=vel, waves=LM.config_waves(cov), seed=1000 * dof + 10 * l + c)
    rep = {}
    bad += LM.run_config(be, bt, nthreads=NTHREADS, report=rep)      # (static modes: the kernel variant launched must be LM.expected_variant's)
    print('full batch: %s: %.1f s %s' % (bt.tag, time.time() - t0, rep), flush=True)
  l, c, n, cov, vel = LM.odd_config(dof)
  if l == lpt:      # per-sample grids of an odd size: the tiled twins on padded tiles
    monkeypatch.setenv('DGP_FORCE_SHAPE', '%d,%d' % (l, c))
    t0 = time.time()
    bt = LM.make(dof, l, c, n, cov, vel=vel, waves=LM.MIN_WAVES, seed=1000 * dof + 10 * l + c + 5, grid=LM.ODD_GRID)
    rep = {}
    bad += LM.run_config(be, bt, nthreads=NTHREADS, report=rep)
    print('full batch: %s: %.1f s %s' % (bt.tag, time.time() - t0, rep), flush=True)
  assert not bad, '%d full-batch failures:\n' % len(bad) + '\n'.join(bad[:80])


@pytest.mark.parametrize('dof', [2, 3])
def test_hip_full_batch_long_trajectories(be, dof, monkeypatch):
  """The loop kernels of gn_long.h (n > 256: one shape, 64 lanes, ceil(n / 64) rows per lane) on 2048 lane-mixed wavefronts: (a)-(d) and (f) as
  above and the directional checks of (e); no autograd sample (the dense oracle at n = 1024 takes minutes), no float64 partial grids for fp32 I/O."""
  monkeypatch.delenv('DGP_FORCE_SHAPE', raising=False)
  bad = []
  for n, cov in ((257, 'static'), (257, 'qfull'), (1024 if dof == 2 else 640, 'perstate')):
    t0 = time.time()
    bt = LM.make(dof, 64, -(-n // 64), n, cov, vel=dof == 2 and cov == 'static', waves=LM.MIN_WAVES, seed=77 + n)
    rep = {}
    bad += LM.run_config(be, bt, nthreads=NTHREADS, report=rep, autograd=False, extra=False, long=True)
    print('full batch: %s: %.1f s %s' % (bt.tag, time.time() - t0, rep), flush=True)
  assert not bad, '%d long-trajectory failures:\n' % len(bad) + '\n'.join(bad[:80])


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('name', sorted(LM.HEADLINE))
def test_hip_headline_ten_iterations_full_size(be, name, io, monkeypatch):
  """Part 3: BASELINE configs[1..3] at B = 4096 x 64 states, 10 GN iterations -- see lane_mix.headline."""
  monkeypatch.delenv('DGP_FORCE_SHAPE', raising=False)
  t0 = time.time()
  bt = LM.headline_batch(name)
  rep = {}
  bad = LM.headline(be, bt, io, nthreads=NTHREADS, report=rep)
  print('headline: %s [%s]: %.1f s %s' % (bt.tag, io, time.time() - t0, rep), flush=True)
  assert not bad, '\n'.join(bad[:40])
