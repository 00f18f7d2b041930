"""GPU (-m gpu): the per-trajectory SPD flag `info` of every kernel family against an inertia reference (tests/spd_cases.py).

`info[b] = 1` is the solver's only failure signal (the reference raises from torch.cholesky there).  It comes from ballots ORed into a 64-bit lane mask
that is cut into trajectory groups at the end of the kernel (SpdCheck, gn_lane.h) -- the construct this project has had compiler trouble with (DESIGN.md
section 7) -- and the rest of the suite only checks 0 on healthy and != 0 on NaN trajectories, plus one case with every trajectory bad by seven orders of
magnitude.  Here, for 2 robots x the 9 forced launch shapes x the 6 covariance modes (lane_mix.configs), the per-sample-grid configuration and the loop
kernels of gn_long.h (n = 257, 640 / 1024), on the lane-mixed batches at 3 wavefronts + a ragged one (B = 14, 7, 3), both I/O types:

  lever A, a ladder of reg (+0.1, then negative rungs that flag some, then all, trajectories; spd_cases.rungs) -- per rung
    (a) info == the long-double C oracle's verdict on every decided trajectory, both directions: dgp_gn_step, dgp_gn_step_errors and the tiled twin where the
        one-launch twins exist, the static kernel variant asserted, Woodbury configurations a second time with DGP_NO_WOODBURY=1;
    (c) the clean trajectories of a negative rung are still solved: dtheta against the oracle at parity_cases.TOL where LAM stays positive definite with reg
        lowered by 5e-6 |max diag(LAM)|;
    (d) the same info per trajectory with the batch rotated by TPW // 2 + 1 (step, fused and traced loop), and for a decided trajectory alone (B = 1);
    (e) dgp_gn_solve / dgp_gn_solve_traced (K = 3, tol_delta the median first-step norm): info == the OR of the reference verdicts at the iterates the
        trajectory itself stepped from (the oracle chained under the stopping rule); whatever the step flags at th_init the loop flags;
  lever B, modes with per-call covariance tensors: one GP block of four chosen trajectories times -50 (first / interior / last lane of a group; wavefront
    slot 0, last, middle, ragged wavefront) -- (a) as above and (b) every other trajectory's dtheta, err, err_ext, info (and unw_*) bit-identical to the batch
    without the negated blocks.
A failure names the configuration, the trajectory, its wavefront and its lane offset."""
import time
import pytest
import harness
import lane_mix as LM
import spd_cases as SC

pytestmark = pytest.mark.gpu
NTHREADS = 16


@pytest.fixture(scope='module')
def be():
  import torch
  assert torch.cuda.is_available(), 'the -m gpu tests need a GPU'
  return harness.Backend('hip')


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('lpt', [16, 32, 64])
@pytest.mark.parametrize('dof', [2, 3])
def test_hip_spd_flag(be, dof, lpt, io, monkeypatch):
  bad = []
  t0 = time.time()
  for cfg, grid, seed in SC.all_configs(dof):
    if cfg[0] != lpt: continue
    if cfg[2] > 256: monkeypatch.delenv('DGP_FORCE_SHAPE', raising=False)      # the loop kernels of gn_long.h choose their own shape
    else: monkeypatch.setenv('DGP_FORCE_SHAPE', '%d,%d' % cfg[:2])
    bt = SC.batch(dof, cfg, grid, seed)
    rep = {}
    bad += SC.run_ladder(be, bt, io, nthreads=NTHREADS, report=rep)
    if cfg[3] in SC.LEVER_B_COVS: bad += SC.run_lever_b(be, bt, io, nthreads=NTHREADS, report=rep)
    print('spd flag: %s [%s]: %s' % (bt.tag, io, rep), flush=True)
  print('spd flag: dof %d lpt %d [%s]: %.1f s' % (dof, lpt, io, time.time() - t0), flush=True)
  assert not bad, '%d SPD-flag failures:\n' % len(bad) + '\n'.join(bad[:80])
