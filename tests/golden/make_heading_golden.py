#!/usr/bin/env python
"""Generate tests/golden/g14_heading_lift.npz: inputs and outputs of the REFERENCE's straight_line_trajb (utils/planner_utils.py:47-56) with dof = 3, imported and run at
generation time (CPU, float64); nothing of its text is stored, only arrays.  This is the only initial trajectory the reference can build for the x-y-heading robot,
and what dgp_heading_lift reproduces as DGP_HEADING_LINEAR + DGP_VEL_KEEP on the planar straight line.

Per case of CASES (n, total_time_sec, B, seed): start and goal configurations (B,1,3) -- x, y inside the limits, headings up to +-7 rad so that several lie outside
(-pi, pi] -- and the trajectory (B,n,6) the reference returns for them.
Re-run with:   python tests/golden/make_heading_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                        # noqa: E402  (where the reference lives, its straight_line_trajb, float64 default)
import make_metrics_golden as MM                # noqa: E402  (write_npz: fixed member timestamps)
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

# n, total_time_sec, B, seed
CASES = ((2, 10.0, 3, 1), (3, 10.0, 3, 2), (17, 7.5, 4, 3), (64, 10.0, 5, 4), (65, 3.0, 2, 5), (130, 10.0, 2, 6))


def main():
  out = {'cases': np.array(['%d %r %d %d' % c for c in CASES])}
  for k, (n, T, B, seed) in enumerate(CASES):
    rs = np.random.RandomState(seed)
    start = np.concatenate([rs.uniform(-4.5, 4.5, (B, 1, 2)), rs.uniform(-7.0, 7.0, (B, 1, 1))], -1)
    goal = np.concatenate([rs.uniform(-4.5, 4.5, (B, 1, 2)), rs.uniform(-7.0, 7.0, (B, 1, 1))], -1)
    th = MG.straight_line_trajb(torch.from_numpy(start), torch.from_numpy(goal), T, n - 1, 3)
    assert th.dtype == torch.float64 and tuple(th.shape) == (B, n, 6)
    out.update({'c%d_start' % k: start, 'c%d_goal' % k: goal, 'c%d_th' % k: th.numpy(), 'c%d_T' % k: np.float64(T)})
  path = os.path.join(HERE, 'g14_heading_lift.npz')
  MM.write_npz(path, out)
  print('wrote %s %.1f KB, %d arrays' % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(out)))


if __name__ == '__main__':
  main()
