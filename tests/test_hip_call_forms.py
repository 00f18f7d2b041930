"""GPU (-m gpu): every kernel instantiation away from the canonical call form -- optional pointers NULL, buffers off the 16-byte boundary (tests/call_forms.py):
2 robots x 2 I/O types x the 9 launch shapes (exact fit and ragged) x the covariance families of tests/test_hip_every_kernel.py, per entry-point group.  The
canonical call is pinned to the oracles; every NULL / alignment form must reproduce it bit for bit, under guard bands and with the inputs left as uploaded.
Why: hipcc has miscompiled the largest instantiations at the join of an `if`, these forms are wave-uniform `if`s around real work, and
PlanLayer runs them on every training step.  A failure names the template arguments and the call form."""
import numpy as np
import pytest
import harness
import call_forms as CF

pytestmark = pytest.mark.gpu
GRIDS = ('per', 'shared1', 'shared16')


@pytest.fixture()
def be():
  import torch
  assert torch.cuda.is_available(), 'the -m gpu tests need a GPU'
  return harness.Backend('hip')


def _finish(be, fails, compared, what):
  print('%s: %d entry-point calls (kernel instantiation x call form), %d comparisons, %d guard-band pairs and %d input buffers checked' %
        (what, be.calls, compared, be.guard_checks, be.input_checks))
  assert be.guard_checks > 0 and be.input_checks > 0 and compared > 0      # the guard bands and the input-immutability checks were live
  assert not fails, '%d call forms differ from the canonical call:\n' % len(fails) + '\n'.join(map(str, fails[:80]))


@pytest.mark.parametrize('group', CF.GROUPS)
@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('dof', [2, 3])
def test_hip_call_forms(be, dof, io, group):
  fails, compared, i = [], 0, 0
  for lpt, c in CF.SHAPES:
    for cov in CF.COVS:
      for n in CF.lengths(lpt, c):
        i += 1
        compared += CF.run_config(be, CF.Cfg(dof, io, (lpt, c), n, cov, grid=GRIDS[i % 3]), (group,), fails)
  if group == 'errs':      # no forced shape: dgp_gn_step_errors as ONE launch (the twins with the errors epilogue, (16,4) up to 64 states and (32,4) up to 128)
    for cov in CF.COVS:
      for n in (64, 61, 128, 125):
        i += 1
        compared += CF.run_config(be, CF.Cfg(dof, io, None, n, cov, grid=GRIDS[i % 3]), (group,), fails)
  _finish(be, fails, compared, 'dof %d %s %s' % (dof, io, group))


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('dof', [2, 3])
def test_hip_call_forms_tiled_grids(be, dof, io):
  """The tiled-grid twins (be.sdf_tiled): built for the shapes (16,4) and (32,4) only (dgp_host.h tiled_shape_ok) -- a forced (64,4) resolves to the twin its
  length selects, so it runs at n = 125 on the (32,4) twin."""
  fails, compared, i = [], 0, 0
  for shape, ns in (((16, 4), (64, 61)), ((32, 4), (128, 125)), ((64, 4), (125,))):
    for n in ns:
      for cov in CF.COVS:
        i += 1
        compared += CF.run_config(be, CF.Cfg(dof, io, shape, n, cov, grid=GRIDS[i % 3], tiled=True), CF.GROUPS, fails, oracle=shape != (64, 4))
  _finish(be, fails, compared, 'dof %d %s tiled grids' % (dof, io))


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_hip_call_forms_long_trajectories(be, io):
  """The loop kernels of gn_long.h at n = 257 (one trajectory per wavefront)."""
  fails, compared = [], 0
  for c in CF.long_configs(io): compared += CF.run_config(be, c, ('forward', 'backward', 'loop'), fails)
  _finish(be, fails, compared, '%s long trajectories' % io)
