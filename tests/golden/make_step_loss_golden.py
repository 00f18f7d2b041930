#!/usr/bin/env python
"""Generate tests/golden/g12_step_loss.npz: the REFERENCE's one_step_loss (learning/train_planner.py:75-120) -- its own text, read from the reference at generation
time and exec'd as make_golden.py::_reference_training_text does (the file as a whole is Python 2 and cannot be imported); nothing of the text is stored, only
arrays -- called the way its training loop calls it (:328): one_step_loss(dthetab, th_opt_b - th_curr_b, qc, obscov, err_sg, err_gp, err_obs, criterion,
learn_params, dof, epoch), dof 2, float64.

For (B, n) in {(1, 2), (3, 16), (5, 17), (7, 33)} and the two weight sets (0.5, 2.0, 0.3) and (0, 1, 1) (vel_loss_lambda, ext_obs_lambda, ext_loss_weight): the
inputs (tests/loss_cases.mixed_batch, shared with the tests), the eight returned terms, and autograd's gradients of 0.5 x total_loss w.r.t. dthetab, th_curr_b,
err_sg, err_gp and err_obs.  Re-run with:   python tests/golden/make_step_loss_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                        # noqa: E402  (where the reference lives, its training text, float64 default)
import make_metrics_golden as MM                # noqa: E402  (write_npz: fixed member timestamps)
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402
sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import loss_cases as LC                         # noqa: E402

SHAPES = ((1, 2), (3, 16), (5, 17), (7, 33))
COTANGENT = 0.5


def main():
  loss_src, _ = MG._reference_training_text()
  ns = {'torch': torch}
  exec(compile(loss_src, '<reference one_step_loss>', 'exec'), ns)
  one_step_loss = ns['one_step_loss']
  out = {'shapes': np.asarray(SHAPES), 'weights': np.asarray(LC.WEIGHTS), 'cotangent': np.float64(COTANGENT)}
  T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  for B, n in SHAPES:
    c = LC.mixed_batch(2, n, B)
    pre = 'B%d_n%d_' % (B, n)
    for k in ('update', 'target', 'target_sub', 'sg', 'gp', 'obs'): out[pre + k] = c[k]
    for wi, (vel_lam, obs_lam, ext_w) in enumerate(LC.WEIGHTS):
      lp = {'optim': {'vel_loss_lambda': vel_lam, 'ext_obs_lambda': obs_lam, 'ext_loss_weight': ext_w}}
      dth, th_curr = T(c['update']).requires_grad_(True), T(c['target_sub']).requires_grad_(True)
      th_opt = T(c['target'])
      e_sg, e_gp, e_obs = T(c['sg']).reshape(B, 1).requires_grad_(True), T(c['gp']).reshape(B, 1, 1).requires_grad_(True), T(c['obs']).reshape(B, 1, 1).requires_grad_(True)
      terms = one_step_loss(dth, th_opt - th_curr, None, None, e_sg, e_gp, e_obs, None, lp, 2, 0)
      grads = torch.autograd.grad(COTANGENT * terms[0], (dth, th_curr, e_sg, e_gp, e_obs))
      w = pre + 'w%d_' % wi
      out[w + 'terms'] = np.array([float(t) for t in terms])
      for name, g in zip(('g_update', 'g_target_sub', 'g_sg', 'g_gp', 'g_obs'), grads): out[w + name] = g.detach().numpy().reshape(c['update'].shape if g.dim() == 3 and g.shape[-1] == 4 else (B,))
  path = os.path.join(HERE, 'g12_step_loss.npz')
  MM.write_npz(path, out)
  print('wrote %s %.1f KB, %d arrays' % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(out)))


if __name__ == '__main__':
  main()
