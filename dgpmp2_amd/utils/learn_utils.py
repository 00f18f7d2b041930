"""The loss of the reference's training loop (learning/train_planner.py:75-120, one_step_loss, called at :328) for this build's outer loops, and the collision
verdict of its initializer training (learning/train_initializer.py:81-88, check_solved).

  one_step_loss_torch  the loss in plain torch ops, this project's own statement of it: runs anywhere (CPU included), differentiable by autograd; the mirror the
                       device loss is tested against and the baseline profiles/tools/step_loss_time.py measures it against;
  one_step_loss        the reference's signature and 8-tuple: on device tensors through dgp_step_loss (include/dgpmp2_hip.h; two launches forward, one backward,
                       one autograd node), otherwise through the mirror.

  check_solved         the reference's signature and Python 0 / 1 for traj[0]: one dgp_sdf_lookup launch on device tensors (and one .item()), the torch mirror otherwise;
  check_solved_batch   the verdict of every trajectory of a batch as a (B,) tensor, nothing synchronised.

Columns: positions are [0, dof), velocities [dof, 2 dof).  For dof 2 these are the columns 0,1 / 2,3 the reference hard-codes; for dof 3 its text would still take
0,1 / 2,3 (theta and v_x as "velocity", v_y and omega ignored) -- its training loop only ever runs dof 2, and this build does not reproduce that."""
import torch

TERM_NAMES = ('total', 'pos', 'vel', 'cov', 'gp', 'sg', 'obs', 'ext')


def _weight(w, key):
  v = w[key]
  return float(v.reshape(-1)[0].item()) if torch.is_tensor(v) else float(v)


def one_step_loss_torch(update, target, err_sg, err_gp, err_obs, weights, dof=None, target_sub=None):
  """-> (total, pos, vel, cov, gp, sg, obs, ext), 0-d tensors.  update, target (B,n,d): the miss is update - target, or update - (target - target_sub);
  pos / vel: the squared miss summed over the position / velocity columns, averaged over trajectories and states; gp, sg, obs: the means of the three errors (None: 0);
  ext = gp + sg + ext_obs_lambda obs; total = pos + vel_loss_lambda vel + ext_loss_weight ext; cov = 0 (the reference's covariance regulariser is commented out).
  weights: a mapping with 'vel_loss_lambda', 'ext_obs_lambda', 'ext_loss_weight' (learn_params['optim'])."""
  dof = update.shape[-1] // 2 if dof is None else int(dof)
  miss = update - (target if target_sub is None else target - target_sub)
  pos = miss[..., :dof].pow(2).sum(-1).mean()
  vel = miss[..., dof:2 * dof].pow(2).sum(-1).mean()
  zero = update.new_zeros(())
  gp, sg, obs = (zero if e is None else e.mean() for e in (err_gp, err_sg, err_obs))
  ext = gp + sg + _weight(weights, 'ext_obs_lambda') * obs
  total = pos + _weight(weights, 'vel_loss_lambda') * vel + _weight(weights, 'ext_loss_weight') * ext
  return total, pos, vel, zero.clone(), gp, sg, obs, ext


def _on_device(t):
  return t.is_cuda


def one_step_loss(th_curr, th_opt, qc_inv_trajb, obscov_inv_traj_b, err_sg, err_gp, err_obs, criterion, learn_params, dof, epoch):
  """The reference's one_step_loss, argument for argument (train_planner.py:75; it is called with th_curr = dthetab and th_opt = th_opt_b - th_curr_b, :328) ->
  (total_loss, pos_loss, vel_loss, cov_loss, gp_loss, sg_loss, obs_loss, ext_loss).  qc_inv_trajb, obscov_inv_traj_b, criterion and epoch are unused, as in the
  reference.  On device tensors: dgp_step_loss in its two-array form (0-d float64 tensors, total differentiable through one backward launch); otherwise
  one_step_loss_torch.  planner.step_loss(dthetab, th_curr_b, th_opt_b, errors) folds the subtraction in as well."""
  weights = learn_params['optim']
  if _on_device(th_curr):
    from .. import _capi
    from ..gpmp2.plan_layer import device_step_loss
    return tuple(device_step_loss(_capi.get_pycall(), int(dof), th_curr, th_opt, None, (err_sg, err_gp, err_obs), weights))
  return one_step_loss_torch(th_curr, th_opt, err_sg, err_gp, err_obs, weights, dof)


def check_solved_batch(trajb, sdfb, robot_radius, cell_size, env_params):
  """check_solved for every trajectory of a batch -> (B,) int64 tensor on trajb's device: 1 where no state of the trajectory has d_obs <= robot_radius at its position
  (columns 0, 1), 0 otherwise.  trajb (B,n,d), read in place; sdfb as utils.sdf_utils.bilinear_interpolate takes it (per-sample grids, one grid or an expand()ed view
  for all, a TiledSdf), of trajb's dtype; cell_size is the `res` of the lookup (the reference passes a cell size taken from im_size, not from the padded width).  On
  device tensors: one launch, no synchronisation; a NaN distance does not block, as in the reference's comparison."""
  from .sdf_utils import sdf_lookup
  from ..gpmp2.sdf_lookup import device_sdf_lookup
  r = _weight({'r': robot_radius}, 'r')
  if trajb.dim() != 3 or trajb.shape[2] < 2: raise ValueError('trajb must be (B,n,d) with d >= 2, got %s' % (tuple(trajb.shape),))
  if _on_device(trajb): out = device_sdf_lookup(sdfb, trajb, cell_size, env_params['x_lims'], env_params['y_lims'], r, want_d=False, want_J=False)
  else: out = sdf_lookup(sdfb, trajb[:, :, :2], cell_size, env_params['x_lims'], env_params['y_lims'], r)
  return (out.raw[:, 0] != 0).to(torch.int64)


def check_solved(traj, sdf, robot_radius, cell_size, env_params, use_cuda=False):
  """The reference's check_solved, argument for argument (train_initializer.py:81): 1 if no state of traj[0] has d_obs <= robot_radius, else 0 -- a Python int (one
  .item(), i.e. one synchronisation on device tensors; check_solved_batch avoids it).  traj (B,n,d): only traj[0] is read, against the first grid of sdf.
  `use_cuda` is unused: the tensors' device decides."""
  return int(check_solved_batch(traj[0:1], sdf[0:1], robot_radius, cell_size, env_params)[0].item())
