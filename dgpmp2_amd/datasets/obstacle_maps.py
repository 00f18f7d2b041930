"""Obstacle maps made on the device: the image generators of the reference's dataset generation.

Reference: datasets/obst_generator.py (generate_rect_obstacle_map :179-221, generate_wall_obstacle_map :226-268) with the parameter sets of
datasets/generate_2d_dataset.py (get_tarpit, get_forest, get_multi_obs, get_passage :29-75).  The reference places the obstacles of one map in a Python rejection loop
that copies and repaints the whole map for every candidate; here every map of a batch is made by ONE launch (dgp_obstacle_maps, csrc/obstacle_maps.hip) with
counter-based randomness: environment number e of a seed is the same map whatever batch it is drawn in.  include/dgpmp2_hip.h states the rule, the reference's quirks
included.  The three trivial generators of generate_2d_im_dataset.py and the saving of images are not part of this build.
"""
import math

import torch

from .. import _capi

INFO_CAPPED, INFO_OVERLAPPING, INFO_WRAPPED = 1, 2, 4      # bits of `info` (include/dgpmp2_hip.h)
DATASET_TYPES = ('tar_pit', 'forest', 'multi_obs', 'passage', 'mixed_clutter')      # generate_2d_dataset.py:26
_KINDS = {'rect': _capi.DGP_OBST_RECT, 'wall': _capi.DGP_OBST_WALL}
_IMAGE_CODES = {torch.uint8: _capi.DGP_U8, torch.float32: _capi.DGP_F32, torch.float64: _capi.DGP_F64}


class ObstacleInfo(object):
  """What dgp_obstacle_maps reports per environment, device tensors: `boxes` (E,64,4) int32 [r0, r1, c0, c1], the slices as painted (zeros past num_boxes),
  `num_boxes` (E,) int32, `draws` (E,64) int32 (the accepted draw index of every obstacle, -1 past the last), `flags` (E,) int32 of INFO_* bits.  The properties are
  small torch ops on the device."""
  __slots__ = ('boxes', 'num_boxes', 'draws', 'flags')

  def __init__(self, boxes, num_boxes, draws, flags): self.boxes, self.num_boxes, self.draws, self.flags = boxes, num_boxes, draws, flags

  @property
  def capped(self): return (self.flags & INFO_CAPPED) != 0

  @property
  def overlapping(self): return (self.flags & INFO_OVERLAPPING) != 0

  @property
  def wrapped(self): return (self.flags & INFO_WRAPPED) != 0


def dataset_params(dataset_type, im_size, start_goal_dist, obstacle_sep):
  """The parameter set of a dataset type exactly as generate_2d_dataset.py:29-75 forms it: a dict with the fields of _capi.DgpObstacleParams -- kind ('rect' / 'wall'),
  n_lo, n_hi (the obstacle count is drawn from [n_lo, n_hi), np.random.randint), w_min, w_max, h_min, h_max, start_x, start_y, end_x, end_y, patch_size, patch_size_obs.
  start_goal_dist is the side of the keep-out patch around a start / goal point (patch_size), obstacle_sep the separation of obstacles (patch_size_obs); for 'passage'
  the third argument is the passage size, as in get_passage: h_min / h_max hold the gap widths and start_y the gap_y of the wall.
  'mixed_clutter' -> a tuple of the sets of 'tar_pit', 'forest' and 'multi_obs', one of which is picked per environment.  The reference's get_mixed_clutter cannot run as
  written -- it calls the three others with the wrong number of arguments (:77-88) --; this is what it evidently means, with both sizes passed on to all three."""
  im_size = int(im_size)
  if dataset_type == 'tar_pit':      # :29-39
    w_min = int(im_size / 10)
    start = int(0.15 * im_size)
    end = int(start + 0.5 * im_size)
    return dict(kind='rect', n_lo=5, n_hi=8, w_min=w_min, w_max=w_min + 1, h_min=w_min, h_max=w_min + 1, start_x=start, start_y=start, end_x=end, end_y=end,
                patch_size=start_goal_dist, patch_size_obs=obstacle_sep)
  if dataset_type == 'forest':       # :41-51
    w_min = int(im_size / 30)
    return dict(kind='rect', n_lo=23, n_hi=45, w_min=w_min, w_max=w_min + 1, h_min=w_min, h_max=w_min + 1, start_x=0, start_y=0, end_x=im_size - 1, end_y=im_size - 1,
                patch_size=start_goal_dist, patch_size_obs=obstacle_sep)
  if dataset_type == 'multi_obs':    # :55-66
    w_min = int(im_size / 8)
    start, end = int(0.1 * im_size), int((1.0 - 0.1) * im_size)
    return dict(kind='rect', n_lo=2, n_hi=5, w_min=w_min, w_max=w_min + 10, h_min=w_min, h_max=w_min + 10, start_x=start, start_y=start, end_x=end, end_y=end,
                patch_size=start_goal_dist, patch_size_obs=obstacle_sep)
  if dataset_type == 'passage':      # :69-75
    w_min, gw_min = int(im_size / 5), int(obstacle_sep)
    return dict(kind='wall', n_lo=1, n_hi=2, w_min=w_min, w_max=w_min + 10, h_min=gw_min, h_max=gw_min + 1, start_x=int(0.15 * im_size), start_y=0, end_x=0, end_y=0,
                patch_size=start_goal_dist, patch_size_obs=0.0)
  if dataset_type == 'mixed_clutter':
    return tuple(dataset_params(t, im_size, start_goal_dist, obstacle_sep) for t in ('tar_pit', 'forest', 'multi_obs'))
  raise ValueError('dataset_type must be one of %s, got %r' % (DATASET_TYPES, dataset_type))


def reference_separations(dataset_type, sphere_radius, epsilon_dist, x_lims, im_size):
  """(start_goal_dist, obstacle_sep) as generate_2d_dataset.py passes them for a dataset type (:151-154, :196-208), from the robot's radius, the obstacle factor's
  epsilon and the cell size."""
  cell_size = (float(x_lims[1]) - float(x_lims[0])) / int(im_size) * 1.0
  safety = int(math.ceil((float(epsilon_dist) + float(sphere_radius)) / cell_size * 1.0))
  robot = int(math.ceil(float(sphere_radius) / cell_size * 1.0))
  table = {'tar_pit': (robot + 2.0 * safety, 0.0), 'forest': (3.0 * robot, 3 * robot), 'multi_obs': (safety + robot, 2.0 * (robot + safety)),
           'passage': (3.0 * robot, 4.0 * robot), 'mixed_clutter': (0.8 * safety, 2.0 * (robot + safety))}
  if dataset_type not in table: raise ValueError('dataset_type must be one of %s, got %r' % (DATASET_TYPES, dataset_type))
  return table[dataset_type]


def confs_to_pixels(confs, x_lims, y_lims, im_size):
  """Start / goal configurations in metres -> pixel coordinates (x, y) as generate_2d_dataset.py:186-192 forms them: the first two columns of `confs` (..., >= 2)
  divided by the cell size, x counted from the left edge and y from the TOP.  -> (..., 2) float64 on the device of `confs`."""
  cell_size = (float(x_lims[1]) - float(x_lims[0])) / int(im_size) * 1.0      # :151
  orig_x, orig_y = -float(x_lims[0]) * 1.0 / cell_size, -float(y_lims[0]) * 1.0 / cell_size
  pts = torch.div(confs[..., :2].to(torch.float64), cell_size)
  return torch.stack((orig_x + pts[..., 0], orig_y - pts[..., 1]), dim=-1)


def _layer(planner_or_layer):
  return getattr(planner_or_layer, 'plan_layer', planner_or_layer)


def _c_params(p, max_draws):
  p = dict(p)
  kind = p.pop('kind')
  if kind not in _KINDS: raise ValueError("kind must be 'rect' or 'wall', got %r" % (kind,))
  p.setdefault('max_draws', max_draws)
  return _capi.Solver.obstacle_params(_KINDS[kind], **p)


def generate_obstacle_maps(planner_or_layer, dataset_type_or_params, num_envs, im_size, seed=0, first_env=0, start_pts=None, goal_pts=None, dtype=torch.uint8,
                           device=None, **params):
  """`num_envs` obstacle maps in one launch.  planner_or_layer: a DiffGPMP2Planner or its PlanLayer.  dataset_type_or_params: one of DATASET_TYPES, or a parameter
  dict as dataset_params returns it, or a sequence of such dicts (one is picked per environment).  im_size: the side of the square maps, or (rows, cols).
  (seed, first_env + e) determine environment e.  start_pts / goal_pts: (E,P,2) device tensors of pixel coordinates (confs_to_pixels), P <= 32, kept free of obstacles
  with a patch around each; a host tensor raises.  dtype: torch.uint8 (1 free / 0 obstacle, what sdf_2d_batch takes), or float32 / float64 (the reference's 1 - count).
  device: where the maps are made when no points say so (default: the current device).
  **params: max_draws (4096) bounds the candidates of one obstacle; start_goal_dist and obstacle_sep, for a dataset type given by name, replace the reference's
  values (reference_separations, from the planner's robot radius, epsilon_dist and limits).
  -> (images (E,1,H,W), ObstacleInfo), device tensors."""
  layer = _layer(planner_or_layer)
  if dtype not in _IMAGE_CODES: raise TypeError('generate_obstacle_maps: uint8, float32 or float64 images, got %s' % dtype)
  H, W = (int(im_size), int(im_size)) if not isinstance(im_size, (tuple, list)) else (int(im_size[0]), int(im_size[1]))
  E = int(num_envs)
  pts, P, dev = [], 0, None
  for name, t in (('start_pts', start_pts), ('goal_pts', goal_pts)):
    if t is None:
      pts.append(None)
      continue
    if not torch.is_tensor(t) or not t.is_cuda:
      raise RuntimeError('dgpmp2_amd.generate_obstacle_maps: `%s` must be a CUDA/ROCm tensor; this build has no CPU path' % name)
    if t.dim() != 3 or t.shape[0] != E or t.shape[2] != 2: raise ValueError('%s must be (%d, P, 2), got %s' % (name, E, tuple(t.shape)))
    if P and t.shape[1] != P: raise ValueError('start_pts and goal_pts must hold the same number of points per environment')
    if dev is not None and t.device != dev: raise RuntimeError('dgpmp2_amd.generate_obstacle_maps: start_pts and goal_pts must share a device')
    P, dev = int(t.shape[1]), t.device
    pts.append(t.detach().to(torch.float64).contiguous())
  if dev is None: dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
  max_draws = int(params.pop('max_draws', 4096))
  if isinstance(dataset_type_or_params, str):
    from ..gpmp2.plan_layer import _f
    sgd, sep = reference_separations(dataset_type_or_params, _f(layer.robot_model.get_sphere_radii()), _f(layer.obs_params['epsilon_dist']),
                                     [_f(v) for v in layer.env_params['x_lims']], W)
    sets = dataset_params(dataset_type_or_params, W, params.pop('start_goal_dist', sgd), params.pop('obstacle_sep', sep))
  else:
    sets = dataset_type_or_params
  if params: raise TypeError('generate_obstacle_maps: unknown parameters %s' % sorted(params))
  if isinstance(sets, dict): sets = (sets,)
  c_sets = [_c_params(p, max_draws) for p in sets]
  solver = layer._solvers.get(torch.float64) or layer._solver(torch.float64)
  images = torch.empty((E, 1, H, W), dtype=dtype, device=dev)
  boxes = torch.empty((E, _capi.DGP_OBST_MAX_BOXES, 4), dtype=torch.int32, device=dev)
  draws = torch.empty((E, _capi.DGP_OBST_MAX_BOXES), dtype=torch.int32, device=dev)
  num_boxes = torch.empty((E,), dtype=torch.int32, device=dev)
  info = torch.empty((E,), dtype=torch.int32, device=dev)
  ptr = lambda t: None if t is None else t.data_ptr()
  with torch.cuda.device(dev):
    solver.obstacle_maps(E, H, W, c_sets, images.data_ptr(), _IMAGE_CODES[dtype], seed=seed, first_env=first_env, start_pts=ptr(pts[0]), goal_pts=ptr(pts[1]), num_pts=P,
                         boxes=boxes.data_ptr(), num_boxes=num_boxes.data_ptr(), draws=draws.data_ptr(), info=info.data_ptr(),
                         stream=torch.cuda.current_stream(dev).cuda_stream)
  return images, ObstacleInfo(boxes, num_boxes, draws, info)
