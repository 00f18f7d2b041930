"""ctypes binding of the C-ABI declared in include/dgpmp2_hip.h.

The product path loads dgpmp2_amd/lib/libdgpmp2_hip.so (built in-tree by __graft_entry__.build()) and
fails loudly when it is missing -- there is no CPU fallback.  The binding class is parameterised by
(library, symbol prefix) only so that the test-suite can drive tests/emul's CPU wavefront emulator,
which exports the same entry points with the prefix `emul_`, through the very same marshalling code.
"""
import ctypes as C
import importlib.util
import os

import torch  # noqa: F401  -- must be imported BEFORE the HIP library is dlopen'ed: torch ships its own libamdhip64.so.7 /
# libhsa-runtime64; loading ours first would bind /opt/rocm's copies and leave the process with two runtimes ("no ROCm-capable
# device" on the first launch).  With torch first, our library's libamdhip64.so.7 dependency resolves to the one already loaded.

DGP_OK, DGP_EINVAL, DGP_EUNSUPPORTED, DGP_EHIP = 0, -1, -2, -3
DGP_F32, DGP_F64, DGP_U8 = 0, 1, 2
DGP_FLAG_NONHOLONOMIC, DGP_FLAG_VEL_LIMITS = 1, 2
DGP_QC_STATIC, DGP_QC_PERSTATE, DGP_QC_QFULL, DGP_QC_SCALAR = 0, 1, 2, 3
DGP_SDF_ROWMAJOR, DGP_SDF_TILED4 = 0, 1
DGP_GSDF_DENSE, DGP_GSDF_DENSE_F64, DGP_GSDF_SPARSE = 0, 1, 2
DGP_ABI_VERSION = 7
DGP_OBST_RECT, DGP_OBST_WALL = 0, 1
DGP_OBST_MAX_BOXES, DGP_OBST_MAX_POINTS, DGP_OBST_MAX_GENERATORS = 64, 32, 4
# columns of dgp_traj_metrics' (B, DGP_METRIC_COUNT) float64 array, in the header's order (DGP_METRIC_*)
METRIC_NAMES = ('avg_vel', 'avg_acc', 'avg_jerk', 'gp_mse', 'in_coll', 'num_penetrating', 'avg_penetration', 'max_penetration', 'coll_intensity',
                'constraint_violation', 'pos_mse', 'vel_mse', 'traj_mse')
DGP_METRIC_COUNT = len(METRIC_NAMES)
# columns of dgp_gp_interpolate's (B, DGP_DENSE_COUNT) float64 summary, in the header's order (DGP_DENSE_*)
DENSE_NAMES = ('in_coll', 'num_colliding', 'avg_penetration', 'max_penetration', 'first_colliding', 'worst_index')
DGP_DENSE_IN_COLL, DGP_DENSE_NUM_COLLIDING, DGP_DENSE_AVG_PENETRATION, DGP_DENSE_MAX_PENETRATION, DGP_DENSE_FIRST_COLLIDING, DGP_DENSE_WORST_INDEX = range(6)
DGP_DENSE_COUNT = len(DENSE_NAMES)
DGP_MAX_NUM_INTER = 1023
DGP_HEADING_LINEAR, DGP_HEADING_TANGENT = 0, 1      # dgp_heading_lift: DgpHeadingParams.heading_mode
DGP_END_SUPPLIED, DGP_END_TANGENT, DGP_END_RANDOM = 0, 1, 2      # ... start_end / goal_end
DGP_VEL_KEEP, DGP_VEL_DIFF = 0, 1      # ... velocity_mode
# dgp_select_samples: status bits of a sample, columns of its (B, DGP_SELECT_COUNT) float64 problem summary in the header's order (DGP_SELECT_*)
DGP_SEL_COLLIDING, DGP_SEL_OUTSIDE, DGP_SEL_NON_FINITE, DGP_SEL_EXCLUDED = 1, 2, 4, 8
SELECT_NAMES = ('solved', 'num_accepted', 'best_index', 'best_score', 'best_max_penetration', 'best_status')
DGP_SELECT_SOLVED, DGP_SELECT_NUM_ACCEPTED, DGP_SELECT_BEST_INDEX, DGP_SELECT_BEST_SCORE, DGP_SELECT_BEST_MAX_PENETRATION, DGP_SELECT_BEST_STATUS = range(6)
DGP_SELECT_COUNT = len(SELECT_NAMES)
DGP_MAX_SELECT_SAMPLES = 1024      # the keys of a problem's samples stay in LDS
DGP_MAX_PRIOR_SAMPLES = 1 << 24      # dgp_prior_samples: the sample index shares a Philox counter word with the stream tag
# entries of dgp_step_loss' (DGP_LOSS_COUNT) float64 terms (one_step_loss's return order) and columns of its (B, DGP_LOSS_PER_TRAJ) float64 per_traj
LOSS_NAMES = ('total', 'pos', 'vel', 'cov', 'gp', 'sg', 'obs', 'ext')
DGP_LOSS_TOTAL, DGP_LOSS_POS, DGP_LOSS_VEL, DGP_LOSS_COV, DGP_LOSS_GP, DGP_LOSS_SG, DGP_LOSS_OBS, DGP_LOSS_EXT = range(8)
DGP_LOSS_COUNT = len(LOSS_NAMES)
LOSS_PER_TRAJ_NAMES = ('pos', 'vel', 'gp', 'sg', 'obs')
DGP_LOSS_PER_TRAJ = len(LOSS_PER_TRAJ_NAMES)
# columns of dgp_sdf_lookup's (B, DGP_LOOKUP_COUNT) float64 summary, in the header's order (DGP_LOOKUP_*)
LOOKUP_NAMES = ('solved', 'num_blocked', 'first_blocked', 'min_dist', 'min_index')
DGP_LOOKUP_SOLVED, DGP_LOOKUP_NUM_BLOCKED, DGP_LOOKUP_FIRST_BLOCKED, DGP_LOOKUP_MIN_DIST, DGP_LOOKUP_MIN_INDEX = range(5)
DGP_LOOKUP_COUNT = len(LOOKUP_NAMES)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DGP_LIB_PATH') or os.path.join(_HERE, 'lib', 'libdgpmp2_hip.so')   # override: tuning builds only


class DgpConfig(C.Structure):
  _fields_ = [('struct_size', C.c_uint32), ('num_states', C.c_int32), ('dof', C.c_int32), ('nlinks', C.c_int32),
              ('io_dtype', C.c_int32), ('flags', C.c_uint32), ('total_time_sec', C.c_double),
              ('x_lims', C.c_double * 2), ('y_lims', C.c_double * 2), ('K_s', C.c_double), ('K_g', C.c_double),
              ('reg', C.c_double), ('sphere_radius', C.c_double), ('Q_c_inv', C.c_double * 9),
              ('cost_sigma', C.c_double), ('epsilon_dist', C.c_double), ('K_d', C.c_double), ('K_v', C.c_double),
              ('v_x', C.c_double), ('v_y', C.c_double)]


class DgpSdf(C.Structure):
  _fields_ = [('data', C.c_void_p), ('rows', C.c_int32), ('cols', C.c_int32), ('batch_stride', C.c_int64), ('layout', C.c_int32),
              ('grad_mode', C.c_int32), ('grad_indices', C.c_void_p)]


class DgpCovs(C.Structure):
  _fields_ = [('qc_mode', C.c_int32), ('qc_inv', C.c_void_p), ('obs_w', C.c_void_p), ('eps', C.c_void_p)]


class DgpSampleParams(C.Structure):
  _fields_ = [('clearance', C.c_double), ('margin', C.c_double), ('min_dist_frac', C.c_double), ('near_tries', C.c_int32), ('max_draws', C.c_int32),
              ('corner_inset', C.c_double)]


class DgpObstacleParams(C.Structure):
  _fields_ = [('kind', C.c_int32), ('n_lo', C.c_int32), ('n_hi', C.c_int32), ('w_min', C.c_int32), ('w_max', C.c_int32), ('h_min', C.c_int32), ('h_max', C.c_int32),
              ('start_x', C.c_int32), ('start_y', C.c_int32), ('end_x', C.c_int32), ('end_y', C.c_int32), ('max_draws', C.c_int32),
              ('patch_size_obs', C.c_double), ('patch_size', C.c_double)]


class DgpPathParams(C.Structure):
  _fields_ = [('clearance', C.c_double), ('max_sweeps', C.c_int32), ('path_cap', C.c_int32)]


class DgpShortcutParams(C.Structure):
  _fields_ = [('clearance', C.c_double), ('check_step', C.c_double), ('path_cap', C.c_int32), ('vertex_cap', C.c_int32), ('lookahead', C.c_int32),
              ('reserved', C.c_int32)]


class DgpHeadingParams(C.Structure):
  _fields_ = [('heading_mode', C.c_int32), ('start_end', C.c_int32), ('goal_end', C.c_int32), ('velocity_mode', C.c_int32), ('blend', C.c_int32), ('reserved', C.c_int32),
              ('seed', C.c_uint64), ('first_problem', C.c_uint64)]


class DgpSelectParams(C.Structure):
  _fields_ = [('struct_size', C.c_uint32), ('num_inter', C.c_int32), ('eps', C.c_double), ('sample_major', C.c_int32), ('require_inside', C.c_int32)]


class DgpLossWeights(C.Structure):
  _fields_ = [('vel_loss_lambda', C.c_double), ('ext_obs_lambda', C.c_double), ('ext_loss_weight', C.c_double)]


class DgpError(RuntimeError):
  def __init__(self, code, msg):
    super(DgpError, self).__init__('dgpmp2_hip error %d: %s' % (code, msg))
    self.code = code


class CApi(object):
  """Thin typed wrapper over one shared library exporting <prefix>create, <prefix>gn_step, ..."""

  SYMBOLS = ('abi_version', 'last_error', 'create', 'destroy', 'num_factor_rows', 'launch_shape', 'step_kernel_variant', 'gn_step', 'gn_solve',
             'eval_errors', 'gn_step_backward', 'eval_errors_backward', 'gn_solve_traced', 'gn_solve_backward', 'gn_step_errors',
             'gn_step_errors_backward', 'sum_partial_grids', 'square_covariances', 'square_covariances_backward', 'sdf_2d_workspace_bytes', 'sdf_2d', 'traj_metrics', 'sample_problems', 'obstacle_maps', 'init_paths', 'shortcut_paths', 'prior_samples', 'prior_launch_shape', 'heading_lift', 'select_samples', 'select_launch_shape', 'gp_interpolate', 'step_loss', 'step_loss_backward', 'sdf_lookup', 'sdf_lookup_backward', 'time_next_launch', 'event_create', 'event_destroy', 'event_elapsed_ms')

  def __init__(self, path, prefix='dgp_'):
    if not os.path.exists(path):
      raise ImportError('%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                        '(hipcc --offload-arch=gfx950).  dgpmp2_amd has no CPU fallback.' % path)
    self.path, self.prefix = path, prefix
    self.lib = C.CDLL(path)
    f = lambda name: getattr(self.lib, prefix + name)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    self.abi_version = f('abi_version'); self.abi_version.restype = C.c_int; self.abi_version.argtypes = []
    self.last_error = f('last_error'); self.last_error.restype = C.c_char_p; self.last_error.argtypes = []
    self.create = f('create'); self.create.restype = C.c_int; self.create.argtypes = [C.POINTER(DgpConfig), C.POINTER(vp)]
    self.destroy = f('destroy'); self.destroy.restype = None; self.destroy.argtypes = [vp]
    self.num_factor_rows = f('num_factor_rows'); self.num_factor_rows.restype = C.c_int; self.num_factor_rows.argtypes = [vp]
    self.launch_shape = f('launch_shape'); self.launch_shape.restype = C.c_int
    self.launch_shape.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    self.step_kernel_variant = f('step_kernel_variant'); self.step_kernel_variant.restype = C.c_int; self.step_kernel_variant.argtypes = [vp, i32]
    self.gn_step = f('gn_step'); self.gn_step.restype = C.c_int
    self.gn_step.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), vp, vp, vp, vp, vp]
    self.gn_solve = f('gn_solve'); self.gn_solve.restype = C.c_int
    self.gn_solve.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), i32, dbl, vp, vp, vp, vp, vp, vp, vp]
    self.eval_errors = f('eval_errors'); self.eval_errors.restype = C.c_int
    self.eval_errors.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), vp, vp, vp, vp, vp, vp]
    self.gn_step_backward = f('gn_step_backward'); self.gn_step_backward.restype = C.c_int
    self.gn_step_backward.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), vp, vp, vp, vp, vp, vp, vp, i64,
                                      i32, vp, vp, vp, vp]
    self.eval_errors_backward = f('eval_errors_backward'); self.eval_errors_backward.restype = C.c_int
    self.eval_errors_backward.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp]
    self.gn_solve_traced = f('gn_solve_traced'); self.gn_solve_traced.restype = C.c_int
    self.gn_solve_traced.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), i32, dbl, vp, vp, vp, vp, vp, vp, vp, vp]
    self.gn_solve_backward = f('gn_solve_backward'); self.gn_solve_backward.restype = C.c_int
    self.gn_solve_backward.argtypes = [vp, i32, vp, vp, C.POINTER(DgpSdf), i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp]
    self.gn_step_errors = f('gn_step_errors'); self.gn_step_errors.restype = C.c_int
    self.gn_step_errors.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), vp, vp, vp, vp, vp, vp, vp, vp]
    self.gn_step_errors_backward = f('gn_step_errors_backward'); self.gn_step_errors_backward.restype = C.c_int
    self.gn_step_errors_backward.argtypes = [vp, i32, vp, vp, vp, C.POINTER(DgpSdf), C.POINTER(DgpCovs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64,
                                             i32, vp, vp, vp, vp, vp]
    self.sum_partial_grids = f('sum_partial_grids'); self.sum_partial_grids.restype = C.c_int
    self.sum_partial_grids.argtypes = [vp, i32, i32, i64, dbl, vp, i32, vp]
    self.square_covariances = f('square_covariances'); self.square_covariances.restype = C.c_int
    self.square_covariances.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    self.square_covariances_backward = f('square_covariances_backward'); self.square_covariances_backward.restype = C.c_int
    self.square_covariances_backward.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    self.sdf_2d_workspace_bytes = f('sdf_2d_workspace_bytes'); self.sdf_2d_workspace_bytes.restype = C.c_size_t
    self.sdf_2d_workspace_bytes.argtypes = [i32, i32, i32, i32]
    self.sdf_2d = f('sdf_2d'); self.sdf_2d.restype = C.c_int
    self.sdf_2d.argtypes = [vp, i32, i32, i32, i32, i32, dbl, vp, i32, i32, vp, C.c_size_t, vp]
    # dgp_traj_metrics: bound only where the library exports it -- tests/emul's CPU emulator (prefix `emul_`) has no twin of the metrics kernel; None otherwise
    self.traj_metrics = getattr(self.lib, prefix + 'traj_metrics', None)
    if self.traj_metrics is not None:
      self.traj_metrics.restype = C.c_int
      self.traj_metrics.argtypes = [vp, i32, vp, C.POINTER(DgpSdf), dbl, vp, vp, vp, vp]
    # dgp_sample_problems: like dgp_traj_metrics, no twin in the emulator
    self.sample_problems = getattr(self.lib, prefix + 'sample_problems', None)
    if self.sample_problems is not None:
      self.sample_problems.restype = C.c_int
      self.sample_problems.argtypes = [vp, i32, C.POINTER(DgpSdf), vp, C.POINTER(DgpSampleParams), C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    # dgp_obstacle_maps: no twin in the emulator either
    self.obstacle_maps = getattr(self.lib, prefix + 'obstacle_maps', None)
    if self.obstacle_maps is not None:
      self.obstacle_maps.restype = C.c_int
      self.obstacle_maps.argtypes = [vp, i32, i32, i32, C.POINTER(DgpObstacleParams), i32, C.c_uint64, C.c_uint64, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    # dgp_init_paths: no twin in the emulator either
    self.init_paths = getattr(self.lib, prefix + 'init_paths', None)
    if self.init_paths is not None:
      self.init_paths.restype = C.c_int
      self.init_paths.argtypes = [vp, i32, C.POINTER(DgpSdf), vp, C.POINTER(DgpPathParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    # dgp_shortcut_paths: no twin in the emulator either
    self.shortcut_paths = getattr(self.lib, prefix + 'shortcut_paths', None)
    if self.shortcut_paths is not None:
      self.shortcut_paths.restype = C.c_int
      self.shortcut_paths.argtypes = [vp, i32, C.POINTER(DgpSdf), vp, C.POINTER(DgpShortcutParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    # dgp_prior_samples: no twin in the emulator either
    self.prior_samples = getattr(self.lib, prefix + 'prior_samples', None)
    self.prior_launch_shape = None
    if self.prior_samples is not None:
      self.prior_samples.restype = C.c_int
      self.prior_samples.argtypes = [vp, i32, i32, vp, vp, vp, dbl, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp]
      self.prior_launch_shape = f('prior_launch_shape'); self.prior_launch_shape.restype = C.c_int
      self.prior_launch_shape.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    # dgp_heading_lift: no twin in the emulator either
    self.heading_lift = getattr(self.lib, prefix + 'heading_lift', None)
    if self.heading_lift is not None:
      self.heading_lift.restype = C.c_int
      self.heading_lift.argtypes = [vp, i32, C.POINTER(DgpHeadingParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    # dgp_select_samples: no twin in the emulator either
    self.select_samples = getattr(self.lib, prefix + 'select_samples', None)
    self.select_launch_shape = None
    if self.select_samples is not None:
      self.select_samples.restype = C.c_int
      self.select_samples.argtypes = [vp, i32, i32, vp, vp, vp, C.POINTER(DgpSdf), vp, C.POINTER(DgpSelectParams), vp, vp, vp, vp, vp, vp, vp]
      self.select_launch_shape = f('select_launch_shape'); self.select_launch_shape.restype = C.c_int
      self.select_launch_shape.argtypes = [vp, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    # dgp_gp_interpolate: no twin in the emulator either
    self.gp_interpolate = getattr(self.lib, prefix + 'gp_interpolate', None)
    if self.gp_interpolate is not None:
      self.gp_interpolate.restype = C.c_int
      self.gp_interpolate.argtypes = [vp, i32, vp, i32, C.POINTER(DgpSdf), dbl, vp, vp, vp, vp]
    # dgp_step_loss / dgp_step_loss_backward: no twin in the emulator either
    self.step_loss = getattr(self.lib, prefix + 'step_loss', None)
    self.step_loss_backward = getattr(self.lib, prefix + 'step_loss_backward', None)
    if self.step_loss is not None:
      self.step_loss.restype = self.step_loss_backward.restype = C.c_int
      self.step_loss.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(DgpLossWeights), vp, vp, vp]
      self.step_loss_backward.argtypes = [i32, i32, i32, i32, vp, vp, vp, C.POINTER(DgpLossWeights), vp, vp, vp, vp, vp, vp, vp, vp]
    # dgp_sdf_lookup / dgp_sdf_lookup_backward: no twin in the emulator either
    self.sdf_lookup = getattr(self.lib, prefix + 'sdf_lookup', None)
    self.sdf_lookup_backward = getattr(self.lib, prefix + 'sdf_lookup_backward', None)
    if self.sdf_lookup is not None:
      self.sdf_lookup.restype = self.sdf_lookup_backward.restype = C.c_int
      self.sdf_lookup.argtypes = [i32, i32, i32, vp, i64, C.POINTER(DgpSdf), dbl, C.POINTER(dbl), C.POINTER(dbl), dbl, vp, vp, vp, vp]
      self.sdf_lookup_backward.argtypes = [i32, i32, i32, vp, i64, C.POINTER(DgpSdf), dbl, C.POINTER(dbl), C.POINTER(dbl), vp, vp, vp, vp, i64, i32, vp]
    self.time_next_launch = f('time_next_launch'); self.time_next_launch.restype = C.c_int; self.time_next_launch.argtypes = [vp, vp]
    self.event_create = f('event_create'); self.event_create.restype = C.c_int; self.event_create.argtypes = [C.POINTER(vp)]
    self.event_destroy = f('event_destroy'); self.event_destroy.restype = None; self.event_destroy.argtypes = [vp]
    self.event_elapsed_ms = f('event_elapsed_ms'); self.event_elapsed_ms.restype = C.c_int
    self.event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
    v = self.abi_version()
    if v != DGP_ABI_VERSION:
      raise ImportError('%s: ABI version %d, binding expects %d' % (path, v, DGP_ABI_VERSION))

  def check(self, rc):
    if rc != DGP_OK:
      raise DgpError(rc, (self.last_error() or b'').decode('utf-8', 'replace'))


class KernelTimer(object):
  """Per-kernel execution times through dgp_time_next_launch: a pool of HIP event pairs, created and read through the library's own
  dgp_event_* helpers (i.e. the HIP runtime the kernels are launched with); `arm()` before a launch makes that launch record its own
  begin / end, `durations_ms()` reads them back after a synchronisation.  Measurement aid for bench.py and the profiling tools --
  not used by the planner."""

  def __init__(self, n, api=None):
    self.api = api if api is not None else get_api()
    self.pairs = []
    for _ in range(n):
      a, b = C.c_void_p(), C.c_void_p()
      self.api.check(self.api.event_create(C.byref(a)))
      self.api.check(self.api.event_create(C.byref(b)))
      self.pairs.append((a, b))
    self.used = 0

  def arm(self):
    a, b = self.pairs[self.used]; self.used += 1
    self.api.check(self.api.time_next_launch(a, b))

  def reset(self):
    self.used = 0

  def durations_ms(self):
    out = []
    for a, b in self.pairs[:self.used]:
      ms = C.c_float()
      self.api.check(self.api.event_elapsed_ms(a, b, C.byref(ms)))
      out.append(ms.value)
    return out

  def __del__(self):
    for a, b in getattr(self, 'pairs', []):
      self.api.event_destroy(a); self.api.event_destroy(b)
    self.pairs = []


_api = None
_pycall = None
import sysconfig
# the trampoline is a CPython extension: its file name carries the interpreter's ABI tag, so that a library built for another Python is
# never loaded by mistake
PYCALL_PATH = os.path.join(_HERE, 'lib', '_dgp_pycall' + (sysconfig.get_config_var('EXT_SUFFIX') or '.so'))
_PYCALL_ENTRIES = ('gn_step', 'gn_solve', 'eval_errors', 'gn_step_backward', 'eval_errors_backward', 'gn_solve_traced', 'gn_solve_backward',
                   'gn_step_errors', 'gn_step_errors_backward', 'sum_partial_grids', 'square_covariances', 'square_covariances_backward', 'traj_metrics', 'gp_interpolate', 'step_loss', 'step_loss_backward', 'sdf_lookup', 'sdf_lookup_backward', 'prior_samples')


def get_api():
  """The product library (HIP).  Raises ImportError if it has not been built."""
  global _api
  if _api is None:
    _api = CApi(LIB_PATH, 'dgp_')
  return _api


class CtypesPycall(object):
  """Drop-in for the trampoline module, on the plain ctypes binding: the same positional signatures (addresses as ints / None, the two
  structs flattened into their seven + four fields), 3-5 us slower per call.  Used when the trampoline has not been built or does not load
  (no Python.h on the build host, another interpreter): the product path is then still the C-ABI, only the marshalling is slower."""

  def __init__(self, api):
    self.api = api

  @staticmethod
  def _sdf(a, i):
    return C.byref(DgpSdf(a[i], int(a[i + 1]), int(a[i + 2]), int(a[i + 3]), int(a[i + 4]), int(a[i + 5]), a[i + 6])) if a[i] else None

  @staticmethod
  def _covs(a, i):
    return C.byref(DgpCovs(int(a[i]), a[i + 1], a[i + 2], a[i + 3]))

  def _prefixed(self, fn, a):
    return fn(a[0], a[1], a[2], a[3], a[4], self._sdf(a, 5), self._covs(a, 12), *a[16:])

  def gn_step(self, *a): return self._prefixed(self.api.gn_step, a)
  def gn_solve(self, *a): return self._prefixed(self.api.gn_solve, a)
  def eval_errors(self, *a): return self._prefixed(self.api.eval_errors, a)
  def gn_step_backward(self, *a): return self._prefixed(self.api.gn_step_backward, a)
  def eval_errors_backward(self, *a): return self._prefixed(self.api.eval_errors_backward, a)
  def gn_solve_traced(self, *a): return self._prefixed(self.api.gn_solve_traced, a)
  def gn_step_errors(self, *a): return self._prefixed(self.api.gn_step_errors, a)
  def gn_step_errors_backward(self, *a): return self._prefixed(self.api.gn_step_errors_backward, a)

  def gn_solve_backward(self, *a):
    return self.api.gn_solve_backward(a[0], a[1], a[2], a[3], self._sdf(a, 4), *a[11:])

  def sum_partial_grids(self, *a): return self.api.sum_partial_grids(*a)
  def square_covariances(self, *a): return self.api.square_covariances(*a)
  def square_covariances_backward(self, *a): return self.api.square_covariances_backward(*a)

  def traj_metrics(self, *a):
    # (handle, batch, th, the seven DgpSdf fields, metric_eps, th_opt, metrics, obs_error, stream)
    return self.api.traj_metrics(a[0], a[1], a[2], self._sdf(a, 3), *a[10:])

  def gp_interpolate(self, *a):
    # (handle, batch, th, num_inter, the seven DgpSdf fields, eps, th_dense, dense_cost, summary, stream)
    return self.api.gp_interpolate(a[0], a[1], a[2], int(a[3]), self._sdf(a, 4), *a[11:])

  def step_loss(self, *a):
    # (dtype, batch, num_states, dof, update, target, target_sub, unw_sg, unw_gp, unw_obs, the three DgpLossWeights fields, terms, per_traj, stream)
    return self.api.step_loss(*a[:10], C.byref(DgpLossWeights(float(a[10]), float(a[11]), float(a[12]))), *a[13:])

  def step_loss_backward(self, *a):
    # (dtype, batch, num_states, dof, update, target, target_sub, the three DgpLossWeights fields, g_total, the six gradient outputs, stream)
    return self.api.step_loss_backward(*a[:7], C.byref(DgpLossWeights(float(a[7]), float(a[8]), float(a[9]))), *a[10:])


  def sdf_lookup(self, *a):
    # (dtype, batch, num_points, points, point_stride, the seven DgpSdf fields, res, x_lo, x_hi, y_lo, y_hi, clearance, d_obs, J, summary, stream)
    return self.api.sdf_lookup(int(a[0]), int(a[1]), int(a[2]), a[3], int(a[4]), self._sdf(a, 5), float(a[12]), (C.c_double * 2)(float(a[13]), float(a[14])),
                               (C.c_double * 2)(float(a[15]), float(a[16])), float(a[17]), *a[18:])

  def sdf_lookup_backward(self, *a):
    # (dtype, batch, num_points, points, point_stride, the seven DgpSdf fields, res, x_lo, x_hi, y_lo, y_hi, g_d, g_J, g_points, g_sdf, g_sdf_batch_stride, g_sdf_copies, stream)
    return self.api.sdf_lookup_backward(int(a[0]), int(a[1]), int(a[2]), a[3], int(a[4]), self._sdf(a, 5), float(a[12]), (C.c_double * 2)(float(a[13]), float(a[14])),
                                        (C.c_double * 2)(float(a[15]), float(a[16])), a[17], a[18], a[19], a[20], int(a[21]), int(a[22]), a[23])

  def prior_samples(self, *a):
    # (handle, batch, num_samples, start, goal, mean, scale, seed, first_problem, noise, th, noise_out, info, stream)
    return self.api.prior_samples(a[0], int(a[1]), int(a[2]), a[3], a[4], a[5], float(a[6]), int(a[7]) & 0xffffffffffffffff, int(a[8]) & 0xffffffffffffffff, *a[9:])


def get_pycall():
  """The METH_FASTCALL trampoline onto the product library's entry points (csrc/dgp_pycall.c): the same C-ABI calls as the ctypes
  binding above at a tenth of the per-call marshalling cost.  What the torch-facing layer (dgpmp2_amd.gpmp2) launches through;
  the ctypes methods of `Solver` stay the reference binding (tests, tools).  The product library itself must exist
  (ImportError otherwise: there is no CPU path); a missing or unloadable trampoline falls back to CtypesPycall with a warning."""
  global _pycall
  if _pycall is None:
    api = get_api()
    try:
      if not os.path.exists(PYCALL_PATH):
        raise ImportError('%s is missing' % PYCALL_PATH)
      spec = importlib.util.spec_from_file_location('_dgp_pycall', PYCALL_PATH)
      mod = importlib.util.module_from_spec(spec)
      spec.loader.exec_module(mod)
      addr = lambda f: C.cast(f, C.c_void_p).value
      mod.bind(*[addr(getattr(api, name)) for name in _PYCALL_ENTRIES])
      _pycall = mod
    except (ImportError, OSError, TypeError) as e:
      import warnings
      warnings.warn('dgpmp2_amd: the call trampoline %s is not usable (%s: %s); using the ctypes binding of the same C-ABI entry points '
                    '(3-5 us more host time per launch).  Build it with `python -c "import __graft_entry__ as g; g.build()"`.'
                    % (os.path.basename(PYCALL_PATH), type(e).__name__, e))
      _pycall = CtypesPycall(api)
  return _pycall


def step_loss(dtype, batch, num_states, dof, update, target, weights, terms, per_traj, target_sub=None, unw_sg=None, unw_gp=None, unw_obs=None, stream=None, api=None):
  """dgp_step_loss (no handle): terms (DGP_LOSS_COUNT) and per_traj (B, DGP_LOSS_PER_TRAJ) float64 from update / target / target_sub (B,n,d) and the three (B) error
  arrays of `dtype` (raw addresses; positions are columns [0, dof), velocities [dof, 2 dof)); weights: a DgpLossWeights or (vel_loss_lambda, ext_obs_lambda,
  ext_loss_weight).  Two stream-ordered launches."""
  api = api if api is not None else get_api()
  if api.step_loss is None:
    raise NotImplementedError('%s does not export %sstep_loss (the CPU emulator has no twin of the loss kernels)' % (api.path, api.prefix))
  w = weights if isinstance(weights, DgpLossWeights) or weights is None else DgpLossWeights(*[float(v) for v in weights])
  api.check(api.step_loss(int(dtype), int(batch), int(num_states), int(dof), update, target, target_sub, unw_sg, unw_gp, unw_obs, C.byref(w) if w is not None else None,
                          terms, per_traj, stream))


def step_loss_backward(dtype, batch, num_states, dof, update, target, weights, target_sub=None, g_total=None, g_update=None, g_target=None, g_target_sub=None,
                       g_unw_sg=None, g_unw_gp=None, g_unw_obs=None, stream=None, api=None):
  """dgp_step_loss_backward (no handle): the gradients of the total loss, scaled by the device scalar *g_total (None: 1.0); every output may be None.  One launch."""
  api = api if api is not None else get_api()
  if api.step_loss_backward is None:
    raise NotImplementedError('%s does not export %sstep_loss_backward (the CPU emulator has no twin of the loss kernels)' % (api.path, api.prefix))
  w = weights if isinstance(weights, DgpLossWeights) or weights is None else DgpLossWeights(*[float(v) for v in weights])
  api.check(api.step_loss_backward(int(dtype), int(batch), int(num_states), int(dof), update, target, target_sub, C.byref(w) if w is not None else None, g_total,
                                   g_update, g_target, g_target_sub, g_unw_sg, g_unw_gp, g_unw_obs, stream))


def _lims(v):
  return None if v is None else (C.c_double * 2)(float(v[0]), float(v[1]))


def sdf_lookup(dtype, batch, num_points, points, point_stride, sdf, res, x_lims, y_lims, clearance=0.0, d_obs=None, J=None, summary=None, stream=None, api=None):
  """dgp_sdf_lookup (no handle): d_obs (B,S) and J (B,S,2) of `dtype` and / or summary (B, DGP_LOOKUP_COUNT) float64 of the bilinear lookup of points (B,S,>=2; row
  pitch point_stride elements) in the grid `sdf` (a DgpSdf), raw addresses.  One launch."""
  api = api if api is not None else get_api()
  if api.sdf_lookup is None:
    raise NotImplementedError('%s does not export %ssdf_lookup (the CPU emulator has no twin of the lookup kernels)' % (api.path, api.prefix))
  api.check(api.sdf_lookup(int(dtype), int(batch), int(num_points), points, int(point_stride), C.byref(sdf) if sdf is not None else None, float(res), _lims(x_lims),
                           _lims(y_lims), float(clearance), d_obs, J, summary, stream))


def sdf_lookup_backward(dtype, batch, num_points, points, point_stride, sdf, res, x_lims, y_lims, g_d=None, g_J=None, g_points=None, g_sdf=None, g_sdf_batch_stride=0,
                        g_sdf_copies=1, stream=None, api=None):
  """dgp_sdf_lookup_backward (no handle): g_points (B,S,2) written, g_sdf accumulated with atomics (zeroed by the caller; sdf.grad_mode DGP_GSDF_DENSE / _F64).  One launch."""
  api = api if api is not None else get_api()
  if api.sdf_lookup_backward is None:
    raise NotImplementedError('%s does not export %ssdf_lookup_backward (the CPU emulator has no twin of the lookup kernels)' % (api.path, api.prefix))
  api.check(api.sdf_lookup_backward(int(dtype), int(batch), int(num_points), points, int(point_stride), C.byref(sdf) if sdf is not None else None, float(res), _lims(x_lims),
                                    _lims(y_lims), g_d, g_J, g_points, g_sdf, int(g_sdf_batch_stride), int(g_sdf_copies), stream))


def make_config(num_states, dof, io_dtype, total_time_sec, x_lims, y_lims, K_s, K_g, reg, sphere_radius, Q_c_inv,
                cost_sigma, epsilon_dist, non_holonomic=False, use_vel_limits=False, K_d=0.0, K_v=0.0, v_x=0.0, v_y=0.0,
                nlinks=1):
  cfg = DgpConfig()
  cfg.struct_size = C.sizeof(DgpConfig)
  cfg.num_states, cfg.dof, cfg.nlinks, cfg.io_dtype = int(num_states), int(dof), int(nlinks), int(io_dtype)
  cfg.flags = (DGP_FLAG_NONHOLONOMIC if non_holonomic else 0) | (DGP_FLAG_VEL_LIMITS if use_vel_limits else 0)
  cfg.total_time_sec = float(total_time_sec)
  cfg.x_lims[0], cfg.x_lims[1] = float(x_lims[0]), float(x_lims[1])
  cfg.y_lims[0], cfg.y_lims[1] = float(y_lims[0]), float(y_lims[1])
  cfg.K_s, cfg.K_g, cfg.reg, cfg.sphere_radius = float(K_s), float(K_g), float(reg), float(sphere_radius)
  q = [float(v) for row in Q_c_inv for v in row]
  if len(q) != int(dof) * int(dof):
    raise ValueError('Q_c_inv must be dof x dof')
  for k in range(9):
    cfg.Q_c_inv[k] = q[k] if k < len(q) else 0.0
  cfg.cost_sigma, cfg.epsilon_dist = float(cost_sigma), float(epsilon_dist)
  cfg.K_d, cfg.K_v, cfg.v_x, cfg.v_y = float(K_d), float(K_v), float(v_x), float(v_y)
  return cfg


class Solver(object):
  """One DgpHandle.  All methods take raw addresses (ints) -- see dgpmp2_amd.gpmp2.plan_layer for the
  torch-facing layer.  Immutable after construction, hence safe to share between streams/threads."""

  def __init__(self, cfg, api=None):
    self.api = api if api is not None else get_api()
    self.cfg = cfg
    h = C.c_void_p()
    self.api.check(self.api.create(C.byref(cfg), C.byref(h)))
    self.handle = h
    self.h = h.value                       # the handle as a plain int (what the trampoline of get_pycall() takes)
    self.M = self.api.num_factor_rows(h)
    self.n, self.dof, self.d = cfg.num_states, cfg.dof, 2 * cfg.dof

  def __del__(self):
    h = getattr(self, 'handle', None)
    if h is not None and h.value:
      self.api.destroy(h)
      self.handle = None

  def launch_shape(self, batch):
    """(lanes per trajectory, states per lane) the kernels will run with for this batch size."""
    l, c = C.c_int32(), C.c_int32()
    self.api.check(self.api.launch_shape(self.handle, int(batch), C.byref(l), C.byref(c)))
    return l.value, c.value

  def step_kernel_variant(self, batch):
    """Kernel variant a static-covariance step of this batch launches: 1 block elimination, 3 / 4 Woodbury interior elimination (num_states fills the shape / does not), 0 general."""
    v = self.api.step_kernel_variant(self.handle, int(batch))
    if v < 0: self.api.check(v)
    return v

  @staticmethod
  def sdf_arg(ptr, rows, cols, batch_stride, layout=DGP_SDF_ROWMAJOR, grad_mode=DGP_GSDF_DENSE, grad_indices=None):
    return DgpSdf(ptr, int(rows), int(cols), int(batch_stride), int(layout), int(grad_mode), grad_indices)

  @staticmethod
  def covs_arg(qc_mode=DGP_QC_STATIC, qc_inv=None, obs_w=None, eps=None):
    return DgpCovs(int(qc_mode), qc_inv, obs_w, eps)

  def gn_step(self, batch, th, start, goal, sdf, covs, dtheta, err=None, err_ext=None, info=None, stream=None):
    self.api.check(self.api.gn_step(self.handle, batch, th, start, goal, C.byref(sdf), C.byref(covs) if covs is not None else None,
                                    dtheta, err, err_ext, info, stream))

  def gn_solve(self, batch, th_init, start, goal, sdf, covs, max_iters, tol_delta, th_out, iters=None, err_hist=None,
               errext_hist=None, err_final=None, info=None, stream=None):
    self.api.check(self.api.gn_solve(self.handle, batch, th_init, start, goal, C.byref(sdf),
                                     C.byref(covs) if covs is not None else None, int(max_iters), float(tol_delta), th_out, iters,
                                     err_hist, errext_hist, err_final, info, stream))

  def eval_errors(self, batch, th, start, goal, sdf, covs, err=None, err_ext=None, unw_sg=None, unw_gp=None, unw_obs=None,
                  stream=None):
    self.api.check(self.api.eval_errors(self.handle, batch, th, start, goal, C.byref(sdf),
                                        C.byref(covs) if covs is not None else None, err, err_ext, unw_sg, unw_gp, unw_obs, stream))

  def gn_step_backward(self, batch, th, start, goal, sdf, covs, dtheta, g_dtheta, g_err_ext, g_th=None, g_start=None, g_goal=None,
                       g_sdf=None, g_sdf_batch_stride=0, g_qc_inv=None, g_obs_w=None, g_eps=None, stream=None, g_sdf_copies=1):
    self.api.check(self.api.gn_step_backward(self.handle, batch, th, start, goal, C.byref(sdf),
                                             C.byref(covs) if covs is not None else None, dtheta, g_dtheta, g_err_ext, g_th, g_start,
                                             g_goal, g_sdf, int(g_sdf_batch_stride), int(g_sdf_copies), g_qc_inv, g_obs_w, g_eps, stream))

  def gn_solve_traced(self, batch, th_init, start, goal, sdf, covs, max_iters, tol_delta, th_out, iters, err_hist=None, errext_hist=None,
                      err_final=None, info=None, th_hist=None, stream=None):
    self.api.check(self.api.gn_solve_traced(self.handle, batch, th_init, start, goal, C.byref(sdf), C.byref(covs) if covs is not None else None,
                                            int(max_iters), float(tol_delta), th_out, iters, err_hist, errext_hist, err_final, info, th_hist, stream))

  def gn_solve_backward(self, batch, start, goal, sdf, max_iters, th_hist, th_out, iters, g_th_out, g_th_init=None, g_start=None, g_goal=None,
                        g_sdf=None, g_sdf_batch_stride=0, stream=None, g_sdf_copies=1):
    self.api.check(self.api.gn_solve_backward(self.handle, batch, start, goal, C.byref(sdf), int(max_iters), th_hist, th_out, iters, g_th_out,
                                              g_th_init, g_start, g_goal, g_sdf, int(g_sdf_batch_stride), int(g_sdf_copies), stream))

  def gn_step_errors(self, batch, th, start, goal, sdf, covs, dtheta, err=None, err_ext=None, info=None, unw_sg=None, unw_gp=None, unw_obs=None,
                     stream=None):
    self.api.check(self.api.gn_step_errors(self.handle, batch, th, start, goal, C.byref(sdf), C.byref(covs) if covs is not None else None,
                                           dtheta, err, err_ext, info, unw_sg, unw_gp, unw_obs, stream))

  def gn_step_errors_backward(self, batch, th, start, goal, sdf, covs, dtheta, g_dtheta, g_err_ext, g_unw_sg, g_unw_gp, g_unw_obs, g_th=None,
                              g_start=None, g_goal=None, g_sdf=None, g_sdf_batch_stride=0, g_qc_inv=None, g_obs_w=None, g_eps=None, workspace=None,
                              stream=None, g_sdf_copies=1):
    self.api.check(self.api.gn_step_errors_backward(self.handle, batch, th, start, goal, C.byref(sdf), C.byref(covs) if covs is not None else None,
                                                    dtheta, g_dtheta, g_err_ext, g_unw_sg, g_unw_gp, g_unw_obs, g_th, g_start, g_goal, g_sdf,
                                                    int(g_sdf_batch_stride), int(g_sdf_copies), g_qc_inv, g_obs_w, g_eps, workspace, stream))

  def traj_metrics(self, batch, th, sdf, metric_eps=0.0, th_opt=None, metrics=None, obs_error=None, stream=None):
    """dgp_traj_metrics: metrics (B, DGP_METRIC_COUNT) float64 and / or obs_error (B, n) of the I/O type, one launch."""
    if self.api.traj_metrics is None:
      raise NotImplementedError('%s does not export %straj_metrics (the CPU emulator has no twin of the metrics kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.traj_metrics(self.handle, batch, th, C.byref(sdf), float(metric_eps), th_opt, metrics, obs_error, stream))

  def gp_interpolate(self, batch, th, num_inter, sdf=None, eps=0.0, th_dense=None, dense_cost=None, summary=None, stream=None):
    """dgp_gp_interpolate: th_dense (B, N_d, d) and dense_cost (B, N_d) of the I/O type and / or summary (B, DGP_DENSE_COUNT) float64, N_d = (n - 1)(num_inter + 1) + 1,
    one launch; sdf may be None when only th_dense is asked for."""
    if self.api.gp_interpolate is None:
      raise NotImplementedError('%s does not export %sgp_interpolate (the CPU emulator has no twin of the interpolation kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.gp_interpolate(self.handle, batch, th, int(num_inter), C.byref(sdf) if sdf is not None else None, float(eps), th_dense, dense_cost, summary, stream))

  @staticmethod
  def sample_params(clearance, margin=0.5, min_dist_frac=0.6, near_tries=15, max_draws=4096, corner_inset=0.2):
    """DgpSampleParams with the constants of generate_optimal_paths_gpmp2.py:58-61, :77-80, :134-145; max_draws bounds the reference's endless loops."""
    return DgpSampleParams(float(clearance), float(margin), float(min_dist_frac), int(near_tries), int(max_draws), float(corner_inset))

  def sample_problems(self, batch, sdf, params, start, goal, th_init, seed=0, first_problem=0, env_index=None, diagonal=None, draws=None, info=None, stream=None):
    """dgp_sample_problems: start / goal (B,1,4) and th_init (B,n,4) of the I/O type, draws (B,2) and info (B) int32, one launch."""
    if self.api.sample_problems is None:
      raise NotImplementedError('%s does not export %ssample_problems (the CPU emulator has no twin of the sampler kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.sample_problems(self.handle, batch, C.byref(sdf) if sdf is not None else None, env_index, C.byref(params) if params is not None else None,
                                            int(seed), int(first_problem), diagonal, start, goal, th_init, draws, info, stream))

  @staticmethod
  def obstacle_params(kind, n_lo, n_hi, w_min, w_max, h_min, h_max, start_x=0, start_y=0, end_x=0, end_y=0, patch_size_obs=0.0, patch_size=0.0, max_draws=4096):
    """DgpObstacleParams: one generator of dgp_obstacle_maps (a wall reads h_min / h_max as its gap widths and start_y as gap_y); max_draws bounds the reference's
    endless loop per obstacle."""
    return DgpObstacleParams(int(kind), int(n_lo), int(n_hi), int(w_min), int(w_max), int(h_min), int(h_max), int(start_x), int(start_y), int(end_x), int(end_y),
                             int(max_draws), float(patch_size_obs), float(patch_size))

  def obstacle_maps(self, batch, rows, cols, params, image, image_dtype=DGP_U8, seed=0, first_env=0, start_pts=None, goal_pts=None, num_pts=0, boxes=None,
                    num_boxes=None, draws=None, info=None, stream=None):
    """dgp_obstacle_maps: image (B,rows,cols) of image_dtype, boxes (B,64,4), num_boxes (B), draws (B,64) and info (B) int32, one launch.  params: one
    DgpObstacleParams or a sequence of them (one is drawn per environment); start_pts / goal_pts: (B,num_pts,2) float64 device arrays or None."""
    if self.api.obstacle_maps is None:
      raise NotImplementedError('%s does not export %sobstacle_maps (the CPU emulator has no twin of the obstacle-map kernel)' % (self.api.path, self.api.prefix))
    if params is None: arr, n = None, 0
    elif isinstance(params, DgpObstacleParams): arr, n = C.pointer(params), 1
    else:
      n = len(params)
      arr = (DgpObstacleParams * max(n, 1))(*params)
    self.api.check(self.api.obstacle_maps(self.handle, int(batch), int(rows), int(cols), arr, n, int(seed), int(first_env), start_pts, goal_pts, int(num_pts), image,
                                          int(image_dtype), boxes, num_boxes, draws, info, stream))

  @staticmethod
  def path_params(clearance, max_sweeps=64, path_cap=0):
    """DgpPathParams: a cell is free where its stored distance exceeds `clearance` (the reference's RRT* validity: sphere_radius + epsilon_dist, ompl_rrtstar.py:18);
    max_sweeps bounds the sweeps of the distance field, path_cap is the second dimension of path_cells."""
    return DgpPathParams(float(clearance), int(max_sweeps), int(path_cap))

  def init_paths(self, batch, sdf, params, start, goal, th_init, field, env_index=None, path_cells=None, num_cells=None, length=None, info=None, stream=None):
    """dgp_init_paths: th_init (B,n,4) of the I/O type from start / goal (B,1,4); field (B,H,W) uint32 (workspace and output); path_cells (B,path_cap), num_cells (B)
    and info (B) int32, length (B) float64; one launch."""
    if self.api.init_paths is None:
      raise NotImplementedError('%s does not export %sinit_paths (the CPU emulator has no twin of the path kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.init_paths(self.handle, batch, C.byref(sdf) if sdf is not None else None, env_index, C.byref(params) if params is not None else None,
                                       start, goal, th_init, field, path_cells, num_cells, length, info, stream))

  @staticmethod
  def shortcut_params(clearance, check_step, path_cap, vertex_cap=0, lookahead=1 << 30):
    """DgpShortcutParams: a point is feasible where its bilinear distance exceeds `clearance`; check_step is the spacing of the check points of a segment (finite,
    >= res / 16); path_cap / vertex_cap are the second dimensions of path_cells / vertex_index; lookahead bounds how far ahead of a vertex a shortcut is tried."""
    return DgpShortcutParams(float(clearance), float(check_step), int(path_cap), int(vertex_cap), int(min(int(lookahead), 1 << 30)), 0)

  def shortcut_paths(self, batch, sdf, params, start, goal, path_cells, num_cells, th, env_index=None, vertex_index=None, num_vertices=None, length=None, info=None,
                     stream=None):
    """dgp_shortcut_paths: th (B,n,4) of the I/O type, in-out, from start / goal (B,1,4) and the path_cells (B,path_cap) / num_cells (B) int32 dgp_init_paths wrote;
    vertex_index (B,vertex_cap), num_vertices (B) and info (B) int32, length (B) float64; one launch."""
    if self.api.shortcut_paths is None:
      raise NotImplementedError('%s does not export %sshortcut_paths (the CPU emulator has no twin of the shortcut kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.shortcut_paths(self.handle, batch, C.byref(sdf) if sdf is not None else None, env_index, C.byref(params) if params is not None else None,
                                           start, goal, path_cells, num_cells, th, vertex_index, num_vertices, length, info, stream))

  def prior_samples(self, batch, num_samples, start, goal, th, mean=None, scale=1.0, seed=0, first_problem=0, noise=None, noise_out=None, info=None, stream=None):
    """dgp_prior_samples: th (B,S,n,d) of the I/O type from start / goal (B,1,d) and mean (B,n,d) or None (the prior mean); noise / noise_out (B,S,n+1,d) float64 or
    None (generated from seed and first_problem / not returned), info (B,S) int32 or None; one launch."""
    if self.api.prior_samples is None:
      raise NotImplementedError('%s does not export %sprior_samples (the CPU emulator has no twin of the sampling kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.prior_samples(self.handle, int(batch), int(num_samples), start, goal, mean, float(scale), int(seed) & 0xffffffffffffffff, int(first_problem) & 0xffffffffffffffff, noise, th, noise_out,
                                          info, stream))

  def prior_launch_shape(self):
    """(lanes per trajectory, 64-state blocks per trajectory) dgp_prior_samples launches for this handle: what its own dispatch reads."""
    if self.api.prior_samples is None:
      raise NotImplementedError('%s does not export %sprior_launch_shape (the CPU emulator has no twin of the sampling kernel)' % (self.api.path, self.api.prefix))
    l, b = C.c_int32(), C.c_int32()
    self.api.check(self.api.prior_launch_shape(self.handle, C.byref(l), C.byref(b)))
    return l.value, b.value

  @staticmethod
  def heading_params(heading_mode=DGP_HEADING_TANGENT, start_end=DGP_END_SUPPLIED, goal_end=DGP_END_SUPPLIED, velocity_mode=DGP_VEL_DIFF, blend=1, seed=0, first_problem=0):
    """DgpHeadingParams: how dgp_heading_lift forms the headings (tangent / the reference's linear rule), each end heading (supplied / the path's own tangent /
    random from (seed, first_problem + b)) and the velocities (finite differences / kept), and over how many rows an end's heading error is blended out (1 .. n - 1)."""
    return DgpHeadingParams(int(heading_mode), int(start_end), int(goal_end), int(velocity_mode), int(blend), 0, int(seed) & 0xffffffffffffffff, int(first_problem) & 0xffffffffffffffff)

  def heading_lift(self, batch, params, th2, start, goal, th, start_heading=None, goal_heading=None, turns_in=None, turns_out=None, info=None, stream=None):
    """dgp_heading_lift (a dof 3 handle): start / goal (B,1,6) and th (B,n,6) of the I/O type from the planar th2 (B,n,4); start_heading / goal_heading (B) and
    turns_in / turns_out (B,n) float64 or None, info (B) int32 or None; one launch."""
    if self.api.heading_lift is None:
      raise NotImplementedError('%s does not export %sheading_lift (the CPU emulator has no twin of the lift kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.heading_lift(self.handle, int(batch), C.byref(params) if params is not None else None, th2, start_heading, goal_heading, turns_in, start, goal, th,
                                         turns_out, info, stream))

  @staticmethod
  def select_params(num_inter=7, eps=0.0, sample_major=False, require_inside=True):
    """DgpSelectParams: K and epsilon of the dense check (as dgp_gp_interpolate), the layout of th / score / exclude ((B,S,..) or sample-major (S,B,..)) and whether a
    sample that leaves the handle's limits is rejected."""
    return DgpSelectParams(C.sizeof(DgpSelectParams), int(num_inter), float(eps), 1 if sample_major else 0, 1 if require_inside else 0)

  def select_samples(self, batch, num_samples, th, params, score=None, exclude=None, sdf=None, env_index=None, th_best=None, best=None, order=None, status=None,
                     sample_summary=None, problem_summary=None, stream=None):
    """dgp_select_samples: per problem the dense check, the total order and the gather of its num_samples optimised trajectories th (B,S,n,d) -- (S,B,n,d) with
    params.sample_major -- of the I/O type; score (I/O type) and exclude (int32) laid out like th's leading axes, or None; sdf with the stride between PROBLEMS'
    grids, or None; outputs th_best (B,n,d), best (B), order / status (B,S) int32, sample_summary (B,S,DGP_DENSE_COUNT) and problem_summary (B,DGP_SELECT_COUNT)
    float64, each or None; one launch."""
    if self.api.select_samples is None:
      raise NotImplementedError('%s does not export %sselect_samples (the CPU emulator has no twin of the selection kernel)' % (self.api.path, self.api.prefix))
    self.api.check(self.api.select_samples(self.handle, int(batch), int(num_samples), th, score, exclude, C.byref(sdf) if sdf is not None else None, env_index,
                                           C.byref(params) if params is not None else None, th_best, best, order, status, sample_summary, problem_summary, stream))

  def select_launch_shape(self, num_samples, num_inter):
    """(lanes per trajectory, wavefronts of a problem's workgroup, passes over the samples) dgp_select_samples launches: what its own dispatch reads."""
    if self.api.select_samples is None:
      raise NotImplementedError('%s does not export %sselect_launch_shape (the CPU emulator has no twin of the selection kernel)' % (self.api.path, self.api.prefix))
    l, w, p = C.c_int32(), C.c_int32(), C.c_int32()
    self.api.check(self.api.select_launch_shape(self.handle, int(num_samples), int(num_inter), C.byref(l), C.byref(w), C.byref(p)))
    return l.value, w.value, p.value

  def eval_errors_backward(self, batch, th, start, goal, sdf, covs, g_err_ext=None, g_unw_sg=None, g_unw_gp=None, g_unw_obs=None,
                           g_th=None, g_start=None, g_goal=None, g_sdf=None, g_sdf_batch_stride=0, g_eps=None, stream=None, g_sdf_copies=1):
    self.api.check(self.api.eval_errors_backward(self.handle, batch, th, start, goal, C.byref(sdf),
                                                 C.byref(covs) if covs is not None else None, g_err_ext, g_unw_sg, g_unw_gp, g_unw_obs,
                                                 g_th, g_start, g_goal, g_sdf, int(g_sdf_batch_stride), int(g_sdf_copies), g_eps, stream))
