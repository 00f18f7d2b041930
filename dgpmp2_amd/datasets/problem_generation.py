"""Planning problems made on the device, and the reference's dataset-generation chain on top of them.

Reference: datasets/generate_optimal_paths_gpmp2.py (get_random_2d_confs :54-81, generate_start_goal :120-162) and datasets/generate_2d_dataset.py (:205-265):
images -> SDFs -> feasible start / goal pairs -> straight-line initial trajectories -> planner.forward() -> collision check -> files.  The reference finds the pairs in
Python rejection loops, one Env2D.is_feasible call per candidate point; here every problem of a batch is sampled by ONE launch (dgp_sample_problems,
csrc/problem_sampler.hip) with counter-based randomness: problem number p of a seed is the same problem whatever batch it is drawn in.  The images are an input, or
made on the device as well (datasets/obstacle_maps.py, dgp_obstacle_maps: the reference's obst_generator.py): generate_dataset then starts from a seed.  RRT*
itself (OMPL) and plotting are not part of this build; the role of the reference's --rrt_star_init -- an initial trajectory that is collision-free where the straight
line is not -- is taken by init_paths (dgp_init_paths, csrc/init_paths.hip): the 5-7 shortest grid path through the free cells, resampled to n states, and
shortcut_paths (dgp_shortcut_paths, csrc/shortcut_paths.hip): that path pulled tight by line of sight, the role of the simplifySolution() call RRTStar.plan makes
(diff_gpmp2/ompl_rrtstar.py:36-41).
"""
import numpy as np
import torch

from .. import _capi
from .planning_dataset import write_environment, write_problem, write_meta

INFO_START_CAP, INFO_GOAL_CAP, INFO_NEAR_TRIES, INFO_DIAGONAL_REPLACED = 1, 2, 4, 8      # bits of `info` (include/dgpmp2_hip.h)


class SampleInfo(object):
  """What dgp_sample_problems reports per problem: `flags` (B,) int32 device tensor of INFO_* bits, `draws` (B,2) int32 device tensor (draw indices of the accepted
  start and goal; -1 for a diagonal problem).  The properties are small torch ops on the device."""
  __slots__ = ('flags', 'draws', 'heading')

  def __init__(self, flags, draws, heading=None): self.flags, self.draws, self.heading = flags, draws, heading      # heading: the HeadingInfo of a dof 3 planner's lift, else None

  @property
  def capped(self): return (self.flags & (INFO_START_CAP | INFO_GOAL_CAP)) != 0

  @property
  def near_tries(self): return (self.flags & INFO_NEAR_TRIES) != 0

  @property
  def diagonal_replaced(self): return (self.flags & INFO_DIAGONAL_REPLACED) != 0


INFO_START_BLOCKED, INFO_GOAL_BLOCKED, INFO_UNREACHABLE, INFO_UNCONVERGED, INFO_PATH_TRUNCATED = 1, 2, 4, 8, 16      # bits of dgp_init_paths' `info`
_FIELD_SCRATCH_BYTES = 1 << 30      # init_paths without return_field: the uint32 distance fields of one launch stay at or below this


class PathInfo(object):
  """What dgp_init_paths reports per problem, device tensors: `flags` (B,) int32 of INFO_* bits, `num_cells` (B,) int32 (cells of the traced path; 0 for a fallback),
  `length` (B,) float64 (arc length of the polyline start -> cells -> goal; the straight distance for a fallback), `path_cells` (B,path_cap) int32 (r * W + c of
  the traced cells, -1 behind them) or None when path_cap is 0, `field` (B,H,W) int32 or None: the BITS of the uint32 cost-to-go field (5 per axis move, 7 per
  diagonal; -1 = 0xffffffff: blocked or unreached) when it was asked for, `shortcut` the ShortcutInfo of init_paths(shortcut=True) or None."""
  __slots__ = ('flags', 'num_cells', 'length', 'path_cells', 'field', 'shortcut', 'heading')

  def __init__(self, flags, num_cells, length, path_cells=None, field=None, shortcut=None, heading=None):
    self.flags, self.num_cells, self.length, self.path_cells, self.field, self.shortcut = flags, num_cells, length, path_cells, field, shortcut
    self.heading = heading      # the HeadingInfo of a dof 3 planner's lift, else None

  @property
  def fell_back(self): return (self.flags & (INFO_START_BLOCKED | INFO_GOAL_BLOCKED | INFO_UNREACHABLE | INFO_UNCONVERGED)) != 0      # th_init is the straight line

  @property
  def unreachable(self): return (self.flags & INFO_UNREACHABLE) != 0

  @property
  def unconverged(self): return (self.flags & INFO_UNCONVERGED) != 0


SHORTCUT_NO_PATH, SHORTCUT_INPUT_TRUNCATED, SHORTCUT_VERTEX_TRUNCATED, SHORTCUT_UNVERIFIED = 1, 2, 4, 8      # bits of dgp_shortcut_paths' `info`
INITS = ('straight', 'grid_path', 'shortcut_path')


class ShortcutInfo(object):
  """What dgp_shortcut_paths reports per problem, device tensors: `flags` (B,) int32 of SHORTCUT_* bits, `num_vertices` (B,) int32 (vertices of the new polyline, the
  start and the goal included; 0 where nothing was simplified), `length` (B,) float64 (its arc length; -1 where nothing was simplified), `vertex_index`
  (B,vertex_cap) int32 (the kept indices into start, traced cells, goal; -1 behind them) or None when vertex_cap is 0 -- SHORTCUT_VERTEX_TRUNCATED is then set for
  every simplified problem and says nothing else."""
  __slots__ = ('flags', 'num_vertices', 'length', 'vertex_index', 'heading')

  def __init__(self, flags, num_vertices, length, vertex_index=None, heading=None):
    self.flags, self.num_vertices, self.length, self.vertex_index, self.heading = flags, num_vertices, length, vertex_index, heading      # heading: as PathInfo's

  @property
  def simplified(self): return (self.flags & (SHORTCUT_NO_PATH | SHORTCUT_INPUT_TRUNCATED)) == 0      # the trajectory was rewritten

  @property
  def unverified(self): return (self.flags & SHORTCUT_UNVERIFIED) != 0      # a kept segment of adjacent vertices is not visible

  @property
  def input_truncated(self): return (self.flags & SHORTCUT_INPUT_TRUNCATED) != 0


PRIOR_OUTSIDE_LIMITS, PRIOR_NON_FINITE = 1, 2      # bits of dgp_prior_samples' `info`


class PriorSampleInfo(object):
  """What dgp_prior_samples reports per sample, device tensors: `flags` (B,S) int32 of PRIOR_* bits, `noise` (B,S,n+1,d) float64: the standard normals the samples
  were made from (row 0 the start, rows 1 .. n-1 the n - 1 intervals, row n the goal observation) when return_noise was set, else None -- feeding them back as
  `noise` reproduces the samples bit for bit."""
  __slots__ = ('flags', 'noise')

  def __init__(self, flags, noise=None): self.flags, self.noise = flags, noise

  @property
  def outside_limits(self): return (self.flags & PRIOR_OUTSIDE_LIMITS) != 0      # a position of the sample leaves x_lims / y_lims (samples are not clamped)

  @property
  def non_finite(self): return (self.flags & PRIOR_NON_FINITE) != 0


def prior_samples(planner_or_layer, startb, goalb, num_samples, seed=0, first_problem=0, mean=None, scale=1.0, noise=None, return_noise=False, dtype=None):
  """Initial trajectories for a multi-start, on the device, one launch: num_samples trajectories per problem drawn from the GP prior the planner optimises under --
  N(mu, Sigma) with Sigma^-1 the matrix of the GN step without obstacle (and non-holonomic / velocity-limit) factors and without reg, mu its solution: smooth
  trajectories from startb to goalb that spread most in the middle.  Gauss-Newton on the hinge cost converges to the local minimum its one initial trajectory
  selects, and the straight line and the grid path both lie on the symmetry axis of an obstacle on their way; a batch of samples does not.  include/dgpmp2_hip.h
  states the exact construction.
  startb, goalb (B,1,d) device tensors.  (seed, first_problem + b, s) determine sample s of problem b, whatever the batch it is drawn in.  mean (B,n,d): the
  trajectory the samples spread around -- None: the prior mean; the th_init of init_paths / shortcut_paths: samples around the grid path.  scale >= 0 multiplies the
  deviation from the mean (0 returns the mean).  noise (B,S,n+1,d) float64: standard normals to use instead of generated ones.  dtype: of the samples, default
  startb's.  Samples are neither clamped nor rejected: info.outside_limits flags those that leave the limits.
  -> (thb (B,S,n,d), info: PriorSampleInfo), device tensors; thb.flatten(0, 1) is what forward() takes."""
  layer = _layer(planner_or_layer)
  for name, t in (('startb', startb), ('goalb', goalb), ('mean', mean), ('noise', noise)):
    if t is not None and (not torch.is_tensor(t) or not t.is_cuda): raise RuntimeError('dgpmp2_amd.prior_samples: `%s` must be a CUDA/ROCm tensor; this build has no CPU path' % name)
  th, noise_out, flags = layer.prior_samples(startb, goalb, num_samples, dtype, mean, scale, seed, first_problem, noise, return_noise)
  return th, PriorSampleInfo(flags, noise_out)


HEADING_ALL_DEGENERATE, HEADING_FILLED, HEADING_SHARP_TURN, HEADING_NON_FINITE = 1, 2, 4, 8      # bits of dgp_heading_lift's `info`
_HEADINGS = {'linear': _capi.DGP_HEADING_LINEAR, 'tangent': _capi.DGP_HEADING_TANGENT}
_ENDS = {'supplied': _capi.DGP_END_SUPPLIED, 'tangent': _capi.DGP_END_TANGENT, 'random': _capi.DGP_END_RANDOM}
_VELOCITIES = {'keep': _capi.DGP_VEL_KEEP, 'diff': _capi.DGP_VEL_DIFF}


class HeadingInfo(object):
  """What dgp_heading_lift reports per trajectory, device tensors: `flags` (B,) int32 of HEADING_* bits, `turns` (B,n) float64: the signed turns the headings were
  summed from (row 0: the direction of the first tangent) when return_turns was set, else None -- feeding them back as `turns` reproduces the lift bit for bit;
  `start`, `goal` (B,1,6): the problem the lift made -- rows 0 and N of its trajectory with zero velocities.  init_paths / shortcut_paths return the trajectory
  only: THESE are the start and goal that belong to it (the goal heading is the representative nearest the path's winding, which may be a full turn away from
  the one the caller passed in, and a tangent end replaces the caller's heading altogether)."""
  __slots__ = ('flags', 'turns', 'start', 'goal')

  def __init__(self, flags, turns=None, start=None, goal=None): self.flags, self.turns, self.start, self.goal = flags, turns, start, goal

  @property
  def all_degenerate(self): return (self.flags & HEADING_ALL_DEGENERATE) != 0      # the path never moves: every heading follows the direction (1, 0)

  @property
  def filled(self): return (self.flags & HEADING_FILLED) != 0                      # some row had no tangent of its own (repeated points) and took an earlier one

  @property
  def sharp_turn(self): return (self.flags & HEADING_SHARP_TURN) != 0              # the path turns by more than a right angle between two rows

  @property
  def non_finite(self): return (self.flags & HEADING_NON_FINITE) != 0


def _mode(table, value, what):
  if value not in table: raise ValueError('%s must be one of %s, got %r' % (what, ', '.join(repr(k) for k in table), value))
  return table[value]


def lift_headings(planner_or_layer, th2b, start_heading=None, goal_heading=None, heading='tangent', ends='supplied', velocity='diff', blend=None, seed=0,
                  first_problem=0, turns=None, return_turns=False):
  """Planar trajectories lifted to problems of the non-holonomic x-y-heading robot (dof 3), on the device, one launch: th2b (B,n,4) -- a straight line of
  sample_problems, a grid path of init_paths, its shortcut -- becomes start, goal (B,1,6) and a trajectory (B,n,6) whose heading follows the path's tangent
  continuously (never wrapped) and is blended into the end headings over `blend` rows, with the path's own central differences as velocities: a trajectory that
  satisfies the non-holonomic factor wherever the path has a tangent.  include/dgpmp2_hip.h states the exact rule.
  heading: 'tangent', or 'linear' -- the reference's rule (straight_line_trajb with dof = 3: linear in time from the start to the goal heading, no wrap).
  ends: 'supplied' (start_heading / goal_heading, (B,) device tensors), 'tangent' (the path's own end tangents; heading='tangent' only) or 'random' (uniform in
  [-pi, pi) from (seed, first_problem + b)), or a (start, goal) pair of those.  velocity: 'diff' (central differences of the stored positions and headings) or 'keep'
  (th2b's velocities and one constant angular velocity: with heading='linear' the reference's trajectory).  blend: default max(1, N // 4), N = n - 1.
  turns (B,n) float64: the signed turns to use instead of generated ones (HeadingInfo.turns of an earlier call).  The goal heading returned is the representative
  of goal_heading nearest the path's own winding (it may lie outside (-pi, pi]); the start heading is start_heading itself.
  -> (startb (B,1,6), goalb (B,1,6), thb (B,n,6), info: HeadingInfo), device tensors of th2b's dtype."""
  layer = _layer(planner_or_layer)
  for name, t in (('th2b', th2b), ('start_heading', start_heading), ('goal_heading', goal_heading), ('turns', turns)):
    if t is not None and (not torch.is_tensor(t) or not t.is_cuda): raise RuntimeError('dgpmp2_amd.lift_headings: `%s` must be a CUDA/ROCm tensor; this build has no CPU path' % name)
  se, ge = (ends, ends) if isinstance(ends, str) else tuple(ends)
  N = int(layer.num_traj_states) - 1
  if blend is None: blend = max(1, N // 4)
  if int(blend) != blend or not 1 <= int(blend) <= N: raise ValueError('blend must be an integer in 1..%d, got %r' % (N, blend))
  hp = _capi.Solver.heading_params(_mode(_HEADINGS, heading, 'heading'), _mode(_ENDS, se, 'ends'), _mode(_ENDS, ge, 'ends'), _mode(_VELOCITIES, velocity, 'velocity'),
                                   int(blend), seed, first_problem)
  if heading == 'linear' and 'tangent' in (se, ge): raise ValueError("ends='tangent' needs heading='tangent': the linear rule forms no tangent")
  for e, t, name in ((se, start_heading, 'start_heading'), (ge, goal_heading, 'goal_heading')):
    if e == 'supplied' and t is None: raise ValueError("ends='supplied' needs `%s` (B,)" % name)
  startb, goalb, thb, turns_out, flags = layer.heading_lift(th2b, hp, None, start_heading if se == 'supplied' else None, goal_heading if ge == 'supplied' else None,
                                                            turns, return_turns)
  return startb, goalb, thb, HeadingInfo(flags, turns_out, startb, goalb)


def _layer(planner_or_layer):
  return getattr(planner_or_layer, 'plan_layer', planner_or_layer)


def _lift_keywords(layer, who, **kw):
  """The heading=, ends=, velocity=, blend= keywords of the planar functions: for a dof 3 layer the given ones as a dict for lift_headings; a dof 2 layer takes none"""
  given = {k: v for k, v in kw.items() if v is not None}
  dof = int(getattr(layer, 'dof', 2))
  if dof == 3: return given
  if given: raise TypeError('dgpmp2_amd.%s: %s only apply to a planner of the x-y-heading robot (dof 3); this one has dof %d' % (who, ', '.join(sorted(given)), dof))
  return None


def _planar_ends(t, name, who):
  """(B,1,6) configurations of the x-y-heading robot -> the (B,1,4) start / goal of the planar kernels and the (B,) float64 headings"""
  if not torch.is_tensor(t) or not t.is_cuda: raise RuntimeError('dgpmp2_amd.%s: `%s` must be a CUDA/ROCm tensor; this build has no CPU path' % (who, name))
  if t.dim() != 3 or tuple(t.shape[1:]) != (1, 6): raise ValueError('dgpmp2_amd.%s: `%s` must be (B,1,6) for a dof 3 planner, got %s' % (who, name, tuple(t.shape)))
  return torch.cat((t[..., :2], torch.zeros_like(t[..., :2])), -1), t[:, 0, 2].to(torch.float64)


def _check_init(init):
  if init not in INITS: raise ValueError("init must be 'straight', 'grid_path' or 'shortcut_path', got %r" % (init,))


def shortcut_paths(planner_or_layer, sdfb, startb, goalb, th_initb, path_info, env_index=None, clearance=None, check_step=None, lookahead=None, vertex_cap=0,
                   heading=None, ends=None, velocity=None, blend=None, _planar=False):
  """Line-of-sight shortcutting of the grid paths of init_paths, on the device, one launch: the traced path of every problem is pulled tight by one greedy pass --
  from a vertex, go to the farthest later vertex that is visible from it -- and resampled to n states like the grid path was: the role of the simplifySolution()
  call RRTStar.plan makes before interpolate() (diff_gpmp2/ompl_rrtstar.py:36-41).  include/dgpmp2_hip.h states the exact rule.
  sdfb, startb, goalb, env_index: as for init_paths, and the same ones.  th_initb (B,n,4), path_info: what init_paths returned for them; path_info.path_cells is
  required (init_paths(path_cap=...) large enough for the longest path: a truncated path is left as it is and flagged).
  clearance: a point is feasible where the bilinear distance exceeds it; default sphere_radius + epsilon_dist, as init_paths.  check_step: the spacing of the check
  points of a segment, default a quarter of a cell.  lookahead: how many vertices ahead a shortcut is tried, default no bound.  vertex_cap > 0 asks for the kept
  indices.
  With no flag but SHORTCUT_VERTEX_TRUNCATED the whole new polyline keeps a distance above clearance - check_step, and it is never longer than the grid path.
  A planner of the x-y-heading robot (dof 3): startb, goalb (B,1,6) and th_initb (B,n,6); their x, y (and planar velocity) columns go through the planar run on
  the layer's planar companion handle, the result through lift_headings with the heading columns of startb / goalb as supplied ends (heading=, ends=, velocity=,
  blend=: lift_headings' keywords, for such a planner only); thb is (B,n,6) and info.heading the HeadingInfo, whose .start / .goal are the start and goal to give
  forward() with thb (the goal heading nearest the NEW path's winding; not the goalb passed in).  The planar run takes th_initb's velocity columns as they are: after
  a velocity='diff' lift those are per-row central differences, not the constant velocities init_paths' planar trajectory had, so a problem the shortcut leaves alone
  (SHORTCUT_NO_PATH, SHORTCUT_INPUT_TRUNCATED) keeps them, and with velocity='keep' so does the result -- init_paths(shortcut=True) runs the whole planar chain
  before its one lift and has no such difference.
  -> (thb (B,n,4): a new tensor, th_initb is not modified; info: ShortcutInfo), device tensors."""
  layer = _layer(planner_or_layer)
  lift = None if _planar else _lift_keywords(layer, 'shortcut_paths', heading=heading, ends=ends, velocity=velocity, blend=blend)
  if lift is not None:
    (s2, hs), (g2, hg) = _planar_ends(startb, 'startb', 'shortcut_paths'), _planar_ends(goalb, 'goalb', 'shortcut_paths')
    if not torch.is_tensor(th_initb) or not th_initb.is_cuda: raise RuntimeError('dgpmp2_amd.shortcut_paths: `th_initb` must be a CUDA/ROCm tensor; this build has no CPU path')
    if th_initb.dim() != 3 or th_initb.shape[-1] != 6: raise ValueError('dgpmp2_amd.shortcut_paths: `th_initb` must be (B,n,6) for a dof 3 planner, got %s' % (tuple(th_initb.shape),))
    th2, info = shortcut_paths(layer, sdfb, s2, g2, torch.cat((th_initb[..., :2], th_initb[..., 3:5]), -1), path_info, env_index, clearance, check_step, lookahead, vertex_cap,
                               _planar=True)
    thb, info.heading = lift_headings(layer, th2, hs, hg, **lift)[2:]
    return thb, info
  if not torch.is_tensor(sdfb) or not sdfb.is_cuda:
    raise RuntimeError('dgpmp2_amd.shortcut_paths: `sdfb` must be a CUDA/ROCm tensor; this build has no CPU path')
  for name, t in (('startb', startb), ('goalb', goalb), ('th_initb', th_initb)):
    if not torch.is_tensor(t) or not t.is_cuda: raise RuntimeError('dgpmp2_amd.shortcut_paths: `%s` must be a CUDA/ROCm tensor; this build has no CPU path' % name)
  if sdfb.dim() == 6:
    raise ValueError('dgpmp2_amd.shortcut_paths reads row-major grids, not 4 x 4 tiles (TiledSdf): pass utils.sdf_utils.untile_sdf(sdfb) or the row-major tensor')
  if path_info is None or path_info.path_cells is None:
    raise ValueError('dgpmp2_amd.shortcut_paths needs the traced cells: call init_paths(..., path_cap=...) and pass its PathInfo')
  if sdfb.dim() == 3: sdfb = sdfb.unsqueeze(1)
  dtype = th_initb.dtype
  if clearance is None:
    from ..gpmp2.plan_layer import _f
    clearance = _f(layer.robot_model.get_sphere_radii()) + _f(layer.obs_params['epsilon_dist'])
  if check_step is None:
    from ..gpmp2.plan_layer import _f
    x_lims = [_f(v) for v in layer.env_params['x_lims']]
    check_step = (x_lims[1] - x_lims[0]) / int(sdfb.shape[-1]) / 4
  cells = path_info.path_cells.contiguous()
  sp = _capi.Solver.shortcut_params(clearance, check_step, int(cells.shape[1]), vertex_cap, (1 << 30) if lookahead is None else lookahead)
  if env_index is not None:
    env_index = env_index.to(torch.int32)
    grids = int(sdfb.shape[0])
    if not (grids == 1 or sdfb.stride(0) == 0) and env_index.is_cuda and not torch.cuda.is_current_stream_capturing():
      lo, hi = torch.aminmax(env_index)
      if int(lo) < 0 or int(hi) >= grids: raise ValueError('env_index must lie in [0, %d), got values in [%d, %d]' % (grids, int(lo), int(hi)))
  thb = th_initb.detach().clone(memory_format=torch.contiguous_format)
  vertex_index, num_vertices, length, flags = layer.shortcut_paths(sdfb, startb, goalb, thb, cells, path_info.num_cells.contiguous(), sp, dtype, env_index)
  return thb, ShortcutInfo(flags, num_vertices, length, vertex_index if vertex_cap > 0 else None)


def init_paths(planner_or_layer, sdfb, startb, goalb, env_index=None, clearance=None, max_sweeps=64, path_cap=0, return_field=False, dtype=None, shortcut=False,
               check_step=None, lookahead=None, heading=None, ends=None, velocity=None, blend=None, _planar=False):
  """Collision-free initial trajectories for a batch of problems, on the device: for every (start, goal) pair the 5-7 shortest path through the free cells of its
  grid, resampled to n states at equal arc length, with the constant velocities of the reference's path_to_traj_avg_vel -- the role of --rrt_star_init
  (generate_optimal_paths_gpmp2.py:95-110).  include/dgpmp2_hip.h states the exact rule.
  sdfb: ROW-MAJOR grids as forward() takes them -- (E,1,H,W) / (E,H,W), or a shared (1,1,H,W) / expand()ed grid; a host tensor raises, and so does a TiledSdf
  (untile_sdf gives the row-major grids back).  startb, goalb (B,1,4).  env_index (B,) integer device tensor: the grid of each problem (checked like sample_problems').
  clearance: a cell is free where its stored distance exceeds it; default sphere_radius + epsilon_dist (ompl_rrtstar.py:18).  max_sweeps bounds the sweeps of the
  distance field (a problem that needs more falls back and is flagged), path_cap > 0 asks for the traced cells, return_field for the (B,H,W) distance fields.
  Without return_field the batch runs in chunks whose uint32 fields stay at or below 1 GiB; a problem's result does not depend on its position or batch, so
  chunking changes nothing.  Problems that fall back (info.fell_back) get the straight line of sample_problems.
  shortcut=True: the grid paths go through shortcut_paths (check_step, lookahead: its parameters, at the same clearance) and th_initb is ITS trajectory -- a short
  any-angle polyline instead of the staircase; info.shortcut is its ShortcutInfo.  With path_cap == 0 the path is then traced with path_cap = min(H W, 4 (H + W))
  (info.path_cells is returned); a problem that fell back, or whose path is longer than that, keeps what it has without shortcut.
  A planner of the x-y-heading robot (dof 3): startb, goalb (B,1,6); their x, y columns go through the planar run on the layer's planar companion handle, and the
  path (shortcut or not) through lift_headings with the heading columns as supplied ends (heading=, ends=, velocity=, blend=: lift_headings' keywords, for such a
  planner only); th_initb is (B,n,6) and info.heading the HeadingInfo, whose .start / .goal are the start and goal to give forward() with th_initb: the goal
  heading is the representative of goalb's nearest the path's own winding, which can lie a full turn from goalb's.
  -> (th_initb (B,n,4), info: PathInfo), device tensors."""
  layer = _layer(planner_or_layer)
  lift = None if _planar else _lift_keywords(layer, 'init_paths', heading=heading, ends=ends, velocity=velocity, blend=blend)
  if lift is not None:
    (s2, hs), (g2, hg) = _planar_ends(startb, 'startb', 'init_paths'), _planar_ends(goalb, 'goalb', 'init_paths')
    th2, info = init_paths(layer, sdfb, s2, g2, env_index, clearance, max_sweeps, path_cap, return_field, dtype, shortcut, check_step, lookahead, _planar=True)
    thb, info.heading = lift_headings(layer, th2, hs, hg, **lift)[2:]
    return thb, info
  if not torch.is_tensor(sdfb) or not sdfb.is_cuda:
    raise RuntimeError('dgpmp2_amd.init_paths: `sdfb` must be a CUDA/ROCm tensor; this build has no CPU path')
  for name, t in (('startb', startb), ('goalb', goalb)):
    if not torch.is_tensor(t) or not t.is_cuda: raise RuntimeError('dgpmp2_amd.init_paths: `%s` must be a CUDA/ROCm tensor; this build has no CPU path' % name)
  if sdfb.dim() == 6:
    raise ValueError('dgpmp2_amd.init_paths reads row-major grids, not 4 x 4 tiles (TiledSdf): pass utils.sdf_utils.untile_sdf(sdfb) or the row-major tensor')
  if sdfb.dim() == 3: sdfb = sdfb.unsqueeze(1)
  if dtype is None: dtype = sdfb.dtype
  if clearance is None:
    from ..gpmp2.plan_layer import _f
    clearance = _f(layer.robot_model.get_sphere_radii()) + _f(layer.obs_params['epsilon_dist'])
  if shortcut:
    if path_cap == 0: path_cap = min(int(sdfb.shape[-2]) * int(sdfb.shape[-1]), 4 * (int(sdfb.shape[-2]) + int(sdfb.shape[-1])))
    th, info = init_paths(layer, sdfb, startb, goalb, env_index, clearance, max_sweeps, path_cap, return_field, dtype, _planar=True)
    th, info.shortcut = shortcut_paths(layer, sdfb, startb, goalb, th, info, env_index, clearance, check_step, lookahead, _planar=True)
    return th, info
  pp = _capi.Solver.path_params(clearance, max_sweeps, path_cap)
  grids, B = int(sdfb.shape[0]), int(startb.shape[0])
  shared = grids == 1 or sdfb.stride(0) == 0
  if env_index is not None:
    env_index = env_index.to(torch.int32)
    if not shared and env_index.is_cuda and not torch.cuda.is_current_stream_capturing():
      lo, hi = torch.aminmax(env_index)
      if int(lo) < 0 or int(hi) >= grids: raise ValueError('env_index must lie in [0, %d), got values in [%d, %d]' % (grids, int(lo), int(hi)))
  H, W = int(sdfb.shape[-2]), int(sdfb.shape[-1])
  chunk = B if return_field else max(1, min(B, _FIELD_SCRATCH_BYTES // (4 * H * W)))
  if chunk >= B:
    th, field, cells, num, length, flags = layer.init_paths(sdfb, startb, goalb, pp, dtype, env_index)
    return th, PathInfo(flags, num, length, cells if path_cap > 0 else None, field if return_field else None)
  parts, scratch = [], torch.empty((chunk, H, W), dtype=torch.int32, device=sdfb.device)
  for b0 in range(0, B, chunk):
    b1 = min(B, b0 + chunk)
    grid = sdfb if (shared or env_index is not None) else sdfb[b0:b1]
    parts.append(layer.init_paths(grid, startb[b0:b1], goalb[b0:b1], pp, dtype, None if env_index is None else env_index[b0:b1], scratch[:b1 - b0]))
  th, cells, num, length, flags = (torch.cat([p[i] for p in parts]) for i in (0, 2, 3, 4, 5))
  return th, PathInfo(flags, num, length, cells if path_cap > 0 else None, None)


def sample_problems(planner_or_layer, sdfb, num_problems=None, env_index=None, clearance=None, seed=0, first_problem=0, diagonal=None, dtype=None, init='straight',
                    heading=None, ends=None, velocity=None, blend=None, **params):
  """Feasible start / goal pairs and straight-line initial trajectories for `num_problems` planning problems, one launch.
  planner_or_layer: a DiffGPMP2Planner or its PlanLayer (dof 2).  sdfb: the signed distance fields as forward() takes them -- (E,1,H,W) (or (E,H,W), what sdf_2d_batch
  returns), a utils.sdf_utils.TiledSdf, or a shared (1,1,H,W) / expand()ed grid; a host tensor raises, like sdf_2d_batch.  num_problems: default one per grid.
  env_index (B,) integer device tensor: the grid each problem is sampled in (probs_per_env > 1 without copies of the grids); its entries are checked against the
  number of grids (one small device -> host copy; not under HIP-graph capture, where the caller vouches for them).  clearance: a point is feasible where its signed
  distance exceeds it; default sphere_radius + epsilon_dist + 0.1 (generate_optimal_paths_gpmp2.py:124).  (seed, first_problem + b) determine problem b.
  diagonal (B,) integer device tensor: -1 random, 0..3 the corner-to-corner problem of :134-145.  dtype: of the outputs, default that of sdfb.
  init: 'straight' (the straight lines of the launch itself), 'grid_path': th_initb is init_paths' for the pairs just sampled, at its default clearance (row-major
  grids only), or 'shortcut_path': init_paths(shortcut=True), the grid path pulled tight by line of sight.
  **params: margin (0.5), min_dist_frac (0.6), near_tries (15), max_draws (4096), corner_inset (0.2) -- _capi.DgpSampleParams.
  A planner of the x-y-heading robot (dof 3): the planar problems are sampled on the layer's planar companion handle and lifted by lift_headings (heading=, ends=,
  velocity=, blend=: its keywords, for such a planner only; ends defaults to 'random' -- the end headings are then a function of (seed, first_problem + b) like the
  points); startb, goalb are (B,1,6), th_initb (B,n,6) and info.heading the HeadingInfo.
  -> (startb (B,1,4), goalb (B,1,4), th_initb (B,n,4), info: SampleInfo), device tensors."""
  layer = _layer(planner_or_layer)
  lift = _lift_keywords(layer, 'sample_problems', heading=heading, ends=ends, velocity=velocity, blend=blend)
  if not torch.is_tensor(sdfb) or not sdfb.is_cuda:
    raise RuntimeError('dgpmp2_amd.sample_problems: `sdfb` must be a CUDA/ROCm tensor; this build has no CPU path')
  if sdfb.dim() == 3: sdfb = sdfb.unsqueeze(1)
  if dtype is None: dtype = sdfb.dtype
  if clearance is None:
    from ..gpmp2.plan_layer import _f
    clearance = _f(layer.robot_model.get_sphere_radii()) + _f(layer.obs_params['epsilon_dist']) + 0.1
  sp = _capi.Solver.sample_params(clearance, **params)
  grids = int(sdfb.shape[0])
  B = int(num_problems) if num_problems is not None else (int(env_index.shape[0]) if env_index is not None else grids)
  if env_index is not None:
    env_index = env_index.to(torch.int32)
    shared = grids == 1 or sdfb.stride(0) == 0
    if not shared and env_index.is_cuda and not torch.cuda.is_current_stream_capturing():
      lo, hi = torch.aminmax(env_index)
      if int(lo) < 0 or int(hi) >= grids: raise ValueError('env_index must lie in [0, %d), got values in [%d, %d]' % (grids, int(lo), int(hi)))
  if diagonal is not None: diagonal = diagonal.to(torch.int32)
  _check_init(init)
  startb, goalb, th_initb, draws, info = layer.sample_problems(sdfb, B, sp, dtype, env_index, diagonal, seed, first_problem)
  if init != 'straight': th_initb = init_paths(layer, sdfb, startb, goalb, env_index=env_index, dtype=dtype, shortcut=init == 'shortcut_path', _planar=True)[0]
  if lift is not None:
    lift.setdefault('ends', 'random')
    if 'supplied' in ((lift['ends'],) if isinstance(lift['ends'], str) else tuple(lift['ends'])):
      raise ValueError("dgpmp2_amd.sample_problems: ends='supplied' has no headings to take here; use 'random' or 'tangent'")
    startb, goalb, th_initb, hinfo = lift_headings(layer, th_initb, seed=seed, first_problem=first_problem, **lift)
    return startb, goalb, th_initb, SampleInfo(info, draws, hinfo)
  return startb, goalb, th_initb, SampleInfo(info, draws)


def generate_dataset(root_dir, mode, images, planner, probs_per_env, seed=0, first_diagonal=True, require_collision_free=True, dataset_type=None, num_envs=None,
                     im_size=None, obstacle_params=None, init='straight', check_inter=0, heading=None, ends=None, velocity=None, blend=None, multistart=0, multistart_scale=1.0, **params):
  """The reference's generation chain for a batch of environments, on the device until the files are written:
    0. images=None: generate_obstacle_maps(planner, dataset_type, num_envs, im_size, seed=seed, **obstacle_params) makes the images (uint8); an environment whose
       map is flagged capped or overlapping is dropped before anything else runs           (generate_2d_dataset.py:194-208; the reference never returns such a map)
    1. sdf_2d_batch(images, padlen=0, res=cell_size)                              (generate_2d_dataset.py:211; cell_size = (x_max - x_min) / image width)
    2. sample_problems: probs_per_env problems per environment; with first_diagonal the first problem of every environment is one of the four diagonals, drawn
       from `seed`                                                                (generate_optimal_paths_gpmp2.py:126-148)
    3. planner.forward on the initial trajectories: the straight lines (init='straight'), init_paths' collision-free grid paths (init='grid_path': the
       reference's --rrt_star_init switch, :95-110, :156-159; generate_2d_dataset.py:225-226), or those paths pulled tight by line of sight
       (init='shortcut_path': init_paths(shortcut=True), the simplifySolution() of ompl_rrtstar.py:36-41)                                       (:181-184)
    4. trajectory_metrics(eps=0): in_coll of every planned trajectory             (generate_2d_dataset.py:247-252)
       check_inter > 0: the verdict is that of the GP-interpolated dense trajectory with check_inter states inside every interval, planner.interpolate(th_opt,
       check_inter, sdfb, eps=0).in_collision -- a trajectory whose support states straddle an obstacle is caught (the reference's 'total_check_step' /
       'use_gp_inter' keys, gpmp2_planner.py:29-41, name this check and nothing implements it); 0, the default: the support states only, as the reference
       multistart = S > 0: steps 3 and 4 are planner.plan_multistart around the initial trajectories -- S samples of the GP prior with mean th_init and spread
       multistart_scale plus th_init itself, the fused loop over all of them, the selection with check_inter states per interval -- th_opt is the chosen
       trajectory and the verdict is `not solved` (no candidate ended free and inside the limits); 0, the default: one start per problem, every output unchanged
    5. write_environment / write_problem / write_meta
  images: (E,H,W) or (E,1,H,W) device tensor, free space > 0.75.  An environment with a problem whose sampling hit max_draws is dropped; so is one with a planned
  trajectory in collision when require_collision_free is set (the reference drops an environment by exception, :247-265).  Written environments are numbered densely.
  A planner of the x-y-heading robot (dof 3) runs the same chain: sample_problems lifts the planar problems (heading=, ends=, velocity=, blend=: lift_headings'
  keywords, for such a planner only; random end headings by default), init_paths lifts its paths with those end headings, 'start' / 'goal' (returned and
  written) are the ones that lift made -- bit for bit rows 0 and N of 'th_init' in x, y and heading -- and the files hold (6,) configurations and (n,6) trajectories.
  **params go to sample_problems.  -> {'num_envs': written, 'kept': [input indices], 'dropped': {input index: reason}, 'start', 'goal', 'th_init', 'th_opt': device
  tensors of ALL E * probs_per_env problems (problem e * probs_per_env + j), 'info': SampleInfo, 'in_coll': (E * probs_per_env,) bool, 'path_info': the PathInfo of
  init_paths (None with init='straight'; with init='shortcut_path' its .shortcut is the ShortcutInfo)}.  With images=None, 'kept' and
  'dropped' count in the num_envs generated environments, E is the number of them that went through the chain, and 'images' (E,1,H,W), 'env_numbers' (their numbers
  among the generated ones) and 'obstacle_info' (ObstacleInfo of all num_envs) are returned as well."""
  from ..utils.sdf_utils import sdf_2d_batch
  if images is None:
    from .obstacle_maps import generate_obstacle_maps
    if dataset_type is None or num_envs is None or im_size is None: raise ValueError('generate_dataset: without images, dataset_type, num_envs and im_size say what to generate')
    gen, oinfo = generate_obstacle_maps(planner, dataset_type, num_envs, im_size, seed=seed, **(obstacle_params or {}))
    capped_h, over_h = oinfo.capped.cpu().numpy(), oinfo.overlapping.cpu().numpy()
    good = [e for e in range(int(num_envs)) if not (capped_h[e] or over_h[e])]
    sel = torch.tensor(good, dtype=torch.long, device=gen.device)
    _check_init(init)
    r = {'num_envs': 0, 'kept': [], 'dropped': {}, 'path_info': None}
    if good:
      r = generate_dataset(root_dir, mode, gen[sel], planner, probs_per_env, seed=seed, first_diagonal=first_diagonal,
                           require_collision_free=require_collision_free, init=init, check_inter=check_inter, heading=heading, ends=ends, velocity=velocity,
                           blend=blend, multistart=multistart, multistart_scale=multistart_scale, **params)
    else:
      write_meta(root_dir, mode, 0, int(probs_per_env), {'x_lims': [float(v) for v in planner.env_params['x_lims']], 'y_lims': [float(v) for v in planner.env_params['y_lims']]},
                 int(gen.shape[-1]))
    r['kept'] = [good[k] for k in r['kept']]
    r['dropped'] = {good[k]: why for k, why in r['dropped'].items()}
    for e in range(int(num_envs)):
      if capped_h[e]: r['dropped'][e] = 'no valid obstacle within max_draws candidates'
      elif over_h[e]: r['dropped'][e] = 'obstacles overlap'
    r.update(images=gen[sel], env_numbers=good, obstacle_info=oinfo)
    return r
  if not torch.is_tensor(images) or not images.is_cuda: raise RuntimeError('dgpmp2_amd.generate_dataset: `images` must be a CUDA/ROCm tensor; this build has no CPU path')
  _check_init(init)
  layer = planner.plan_layer
  im = images[:, 0] if images.dim() == 4 else images
  E, H, W = im.shape
  P = int(probs_per_env)
  x_lims, y_lims = [float(v) for v in planner.env_params['x_lims']], [float(v) for v in planner.env_params['y_lims']]
  cell_size = (x_lims[1] - x_lims[0]) / W
  sdf = sdf_2d_batch(im, padlen=0, res=cell_size).unsqueeze(1)      # (E,1,H,W) float64
  B = E * P
  env_index = torch.arange(E, device=im.device, dtype=torch.int32).repeat_interleave(P)
  diagonal = torch.full((B,), -1, dtype=torch.int32, device=im.device)
  if first_diagonal: diagonal[::P] = torch.from_numpy(np.random.RandomState(seed).randint(0, 4, E).astype(np.int32)).to(im.device)
  lift = _lift_keywords(layer, 'generate_dataset', heading=heading, ends=ends, velocity=velocity, blend=blend) or {}
  startb, goalb, th_initb, info = sample_problems(layer, sdf, B, env_index=env_index, seed=seed, diagonal=diagonal, **lift, **params)
  path_info = None
  if init != 'straight':
    if 'ends' in lift:      # the end headings are those sample_problems drew: random ones arrive as supplied
      pair = (lift['ends'], lift['ends']) if isinstance(lift['ends'], str) else tuple(lift['ends'])
      lift = dict(lift, ends=tuple('supplied' if e == 'random' else e for e in pair))
    th_initb, path_info = init_paths(layer, sdf, startb, goalb, env_index=env_index, shortcut=init == 'shortcut_path', **lift)
    if path_info.heading is not None: startb, goalb = path_info.heading.start, path_info.heading.goal      # rows 0 and N of th_initb: the goal heading nearest THIS path's winding
  sdfb = sdf.index_select(0, env_index.long())      # one grid per problem, what forward() takes
  imb = (im > 0.75).to(sdf.dtype).unsqueeze(1).index_select(0, env_index.long())
  multi = None
  with torch.no_grad():
    if int(multistart) > 0:
      th_opt, multi = planner.plan_multistart(startb, goalb, sdfb, int(multistart), th_extra=th_initb[:, None], seed=seed, mean=th_initb, scale=multistart_scale,
                                              num_inter=int(check_inter), eps=0.0)
      in_coll = ~multi.select.solved
    else: th_opt = planner.forward(th_initb, startb, goalb, imb, sdfb)[0]
    if multi is not None: pass
    elif int(check_inter) > 0: in_coll = planner.interpolate(th_opt, int(check_inter), sdfb, eps=0.0).in_collision
    else: in_coll = planner.trajectory_metrics(th_opt, sdfb, eps=0.0).in_collision
  capped_h, coll_h = info.capped.view(E, P).any(1).cpu().numpy(), in_coll.view(E, P).any(1).cpu().numpy()
  s_h, g_h, th_h = startb.cpu().numpy(), goalb.cpu().numpy(), th_opt.cpu().numpy()
  im_h, sdf_h = (im > 0.75).to(torch.float64).cpu().numpy(), sdf[:, 0].cpu().numpy()
  kept, dropped = [], {}
  for e in range(E):
    if capped_h[e]: dropped[e] = 'no feasible start / goal pair within max_draws candidates'
    elif require_collision_free and coll_h[e]: dropped[e] = 'Trajectory is in collision'
    else:
      k = len(kept)
      write_environment(root_dir, mode, k, im_h[e], sdf_h[e])
      for j in range(P):
        b = e * P + j
        write_problem(root_dir, mode, k, j, s_h[b], g_h[b], th_h[b])
      kept.append(e)
  write_meta(root_dir, mode, len(kept), P, {'x_lims': x_lims, 'y_lims': y_lims}, W)
  return {'num_envs': len(kept), 'kept': kept, 'dropped': dropped, 'start': startb, 'goal': goalb, 'th_init': th_initb, 'th_opt': th_opt, 'info': info,
          'in_coll': in_coll, 'path_info': path_info, **({'multistart': multi} if multi is not None else {})}
