#!/usr/bin/env python
"""Generate tests/golden/g13_sdf_lookup.npz: the REFERENCE's bilinear_interpolate (utils/sdf_utils.py:38-107), imported and run at generation time (CPU, float64)
with autograd through BOTH outputs, and its check_solved (learning/train_initializer.py:81-88) -- that function's own text, read from the reference and exec'd as
make_golden.py::_reference_training_text does (the file as a whole cannot be imported); nothing of the text is stored, only arrays.

Per case of CASES (tests/lookup_cases.py supplies grids, frames, points and cotangents, shared with the tests): the points, d_obs, J, autograd's gradients of
sum(g_d d_obs) + sum(g_J J) w.r.t. the points and the grids (a shared grid: w.r.t. the one grid behind the expand()ed view), a clearance -- the smallest d_obs of
the middle row, so that row ties and the others split -- and the reference's check_solved verdict of every row at that clearance.  The grids of the 40 x 32 cases are fixture
g1_factors_2d's and are not stored again.  One float32 case records the dtypes the reference returns.
Re-run with:   python tests/golden/make_lookup_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                        # noqa: E402  (where the reference lives, its bilinear_interpolate, float64 default)
import make_metrics_golden as MM                # noqa: E402  (write_npz: fixed member timestamps)
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402
sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import lookup_cases as LC                       # noqa: E402

# name, frame, B, S, shared grid
CASES = (('a', '5x7', 3, 17, False), ('b', '2x2', 1, 33, False), ('c', 'g1', 5, 16, False), ('d', 'g1_cell', 3, 33, True), ('e', '5x7', 5, 3, True), ('f', '2x2', 3, 1, False))


def _reference_check_solved():
  lines = open(os.path.join(MG.REF, 'diff_gpmp2/learning/train_initializer.py')).read().split('\n')
  i0 = next(i for i, l in enumerate(lines) if l.startswith('def check_solved'))
  i1 = next(i for i, l in enumerate(lines) if i > i0 and l.startswith('def '))
  ns = {'torch': torch, 'bilinear_interpolate': MG.bilinear_interpolate}
  exec(compile('\n'.join(lines[i0:i1]), '<reference check_solved>', 'exec'), ns)
  return ns['check_solved']


def main():
  check_solved = _reference_check_solved()
  T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  env = {'x_lims': list(LC.X_LIMS), 'y_lims': list(LC.Y_LIMS)}
  out = {'cases': np.array(['%s %s %d %d %d' % c for c in CASES])}
  for name, frame, B, S, shared in CASES:
    gname, res = LC.FRAMES[frame]
    grid = LC.grids(gname, 1 if shared else B)
    pts = LC.points(frame, B, S)
    g_d, g_J = LC.cotangents(B, S)
    base = T(grid).requires_grad_(True)
    imb = base.expand(B, -1, -1) if shared else base
    st = T(pts).requires_grad_(True)
    d, J = MG.bilinear_interpolate(imb.unsqueeze(1), st, res, env['x_lims'], env['y_lims'])
    g_imb, g_st = torch.autograd.grad((d[:, :, 0] * T(g_d)).sum() + (J * T(g_J)).sum(), (base, st))
    clearance = float(d[B // 2].min())
    traj = torch.cat([st.detach(), torch.zeros(B, S, 2)], -1)
    verdicts = [check_solved(traj[b:b + 1], imb.detach()[b:b + 1].unsqueeze(1), clearance, res, env, False) for b in range(B)]
    pre = name + '_'
    if gname != 'g1': out[pre + 'grid'] = grid
    out.update({pre + 'points': pts, pre + 'd_obs': d.detach().numpy(), pre + 'J': J.detach().numpy(), pre + 'g_points': g_st.numpy(), pre + 'g_grid': g_imb.numpy(),
                pre + 'clearance': np.float64(clearance), pre + 'solved': np.asarray(verdicts, np.int64)})
  # what the reference returns for float32 inputs
  grid, pts = LC.grids('5x7', 1).astype(np.float32), LC.points('5x7', 1, 3).astype(np.float32)
  torch.set_default_dtype(torch.float32)      # torch's stock default, which a user of the reference runs under (make_golden sets float64 for everything else)
  try: d, J = MG.bilinear_interpolate(T(grid).unsqueeze(1), T(pts), LC.FRAMES['5x7'][1], env['x_lims'], env['y_lims'])
  finally: torch.set_default_dtype(torch.float64)
  out.update({'f32_points': pts, 'f32_d_obs': d.numpy(), 'f32_J': J.numpy(), 'f32_dtypes': np.array([str(d.dtype), str(J.dtype)])})
  path = os.path.join(HERE, 'g13_sdf_lookup.npz')
  MM.write_npz(path, out)
  print('wrote %s %.1f KB, %d arrays' % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(out)))


if __name__ == '__main__':
  main()
