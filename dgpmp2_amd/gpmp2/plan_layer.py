"""PlanLayer -- host-side mirror of the reference's diff_gpmp2.gpmp2.plan_layer.PlanLayer (plan_layer.py:13-99).

Same constructor arguments, same forward() signature and return tuple, same public helpers; the body of forward() --
factor evaluation, linear-system assembly, solve, the two error evaluations -- is ONE launch of the fused HIP kernel
behind the C-ABI (include/dgpmp2_hip.h: dgp_gn_step), and its autograd backward is ONE launch of
dgp_gn_step_backward.  Nothing of the reference's dense A/b/K/mask machinery exists here.

Differences a caller can observe (all deliberate):
  * tensors must live on a CUDA (ROCm) device; there is no CPU path (the reference's use_cuda=False runs on CPU);
  * float32 and float64 tensors are both accepted (the reference only works in float64); arithmetic inside
    the kernel is float64 either way;
  * the batch size is NOT baked in at construction: any leading dimension works with one PlanLayer;
  * forward() itself is re-entrant (all inputs are arguments; the C-ABI handle is immutable).  Only for the reference's
    error_batch(thb, sdfb)-style helpers does the layer remember the means/covariances of the last forward();
  * a non-SPD system raises RuntimeError (as torch.cholesky does in the reference) only when `check_spd` is True,
    because the check forces a device synchronisation; the per-trajectory flags are always available in `last_info`.
    When no input requires grad (planning loops) `last_info` is ONE buffer per (batch, device, stream), overwritten by the next
    forward() on that stream -- clone() it to keep an iteration's flags; a differentiable step or check_spd gets its own tensor;
  * the autograd node of forward() holds plain references to its inputs (addresses + a version-counter check instead of
    SavedVariables, ~1.5 us per tensor): they are released with the node, not at the end of backward(), and
    torch.autograd.graph.saved_tensors_hooks (save_on_cpu, checkpointing) do not see them -- only `dtheta` is a SavedVariable;
  * a `qc_inv_trajb` tensor that DiffGPMP2Planner.get_covariances built in the 'diag_identity' mode carries its n - 1 scalars as a tag (and its version counter: an
    in-place edit voids it); forward() / forward_with_errors() and their backward then launch the scaled-mask static kernels (DGP_QC_SCALAR) instead of the per-state
    ones.  Same values to rounding, the gradient returned for the tensor is that of its dof x dof blocks either way; a copy of the tensor (no tag) takes the per-state path.
"""
import collections
import weakref

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _capi


def _f(x):
  """python float from a float / 0-d or 1-element tensor / 1-element list."""
  if torch.is_tensor(x):
    return float(x.reshape(-1)[0].item())
  if isinstance(x, (list, tuple)):
    return _f(x[0])
  return float(x)


def _io_code(dtype):
  if dtype == torch.float32: return _capi.DGP_F32
  if dtype == torch.float64: return _capi.DGP_F64
  raise TypeError('dgpmp2_amd supports float32 and float64 tensors, got %s' % dtype)


def solver_config(num_states, dof, io_dtype, total_time_sec=10.0, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0), K_s=0.01, K_g=0.01,
                  reg=0.1, sphere_radius=0.4, Q_c_inv=None, cost_sigma=0.01, epsilon_dist=0.4, **kw):
  """DgpConfig with the defaults of the reference's examples/configs/{gpmp2_2d_params,robot_2d,env_2d_params}.yaml."""
  if Q_c_inv is None:
    Q_c_inv = [[1.0 if i == j else 0.0 for j in range(dof)] for i in range(dof)]
  return _capi.make_config(num_states=num_states, dof=dof, io_dtype=_io_code(io_dtype), total_time_sec=total_time_sec,
                           x_lims=x_lims, y_lims=y_lims, K_s=K_s, K_g=K_g, reg=reg, sphere_radius=sphere_radius, Q_c_inv=Q_c_inv,
                           cost_sigma=cost_sigma, epsilon_dist=epsilon_dist, **kw)


_SDF_GRAD_COPIES = 8      # MI355X has 8 XCDs, each with its own L2: one FLOAT64 partial grid per XCD (XCD-local atomics; summed afterwards by dgp_sum_partial_grids).  (Two per XCD -- round 4's fp32 choice -- run the backward kernel no faster with double grids and double the zero fill and the sum: 27.7 vs 27.5 us, profiles/tools/ubench.py --what bwd_sdf16w,bwd_sdf8w --covs perstate)
_ALL_STATIC = (True, True, True)
_NO_COVS = (_capi.DGP_QC_STATIC, None, None, None)       # the four fields of DgpCovs as the trampoline takes them

# current device / current raw stream as plain ints: torch.cuda.current_stream() builds a Stream object (1.2 us), the private getters
# are what it calls underneath (0.1 us each); fall back to the public API where a torch build lacks them
_cur_dev = getattr(torch._C, '_cuda_getDevice', None) or torch.cuda.current_device
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None) or (lambda i: torch.cuda.current_stream(i).cuda_stream)


def _require_cuda(t, name):
  if not t.is_cuda:
    raise RuntimeError('dgpmp2_amd: `%s` must be a CUDA/ROCm tensor (got device %s); this build has no CPU path' % (name, t.device))


def _same_device(dev, **named):
  """Every tensor argument must live on the device of `thb` (index `dev`): the kernel receives raw addresses."""
  for name, t in named.items():
    if t is not None and t.get_device() != dev:
      raise RuntimeError('dgpmp2_amd: `%s` is on %s but `thb` is on cuda:%d; all inputs of one call must share a device' % (name, t.device, dev))


def _ptr(t):
  return None if t is None else t.data_ptr()


def _launch(dev, fn, *args):
  """One C-ABI call through the trampoline with cuda:`dev` as the current device; a non-zero status raises DgpError."""
  if dev == _cur_dev():
    rc = fn(*args)
  else:
    with torch.cuda.device(dev):
      rc = fn(*args)
  if rc:
    _capi.get_api().check(rc)


def _expand_base(t):
  """sdfb as autograd should see it.  A shared grid usually arrives as `grid.expand(B, 1, H, W)` of a (1, 1, H, W) tensor: differentiating w.r.t. the
  expanded view makes autograd's ExpandBackward sum B slices of whatever the node returns -- 4096 x 65536 elements, 45 us on MI355X, for a sum the
  backward kernel has already formed.  When `t` is exactly such a view the node takes the view's BASE as its differentiable input (same storage, same
  launch) and returns the (1, 1, H, W) gradient itself.  Anything else (a view of a view, a differently strided base) is returned unchanged and gets B
  equal shares (see _SdfGrad.finish)."""
  if t is None or t.dim() not in (4, 6) or t.shape[0] <= 1 or t.stride(0) != 0 or not t._is_view(): return t
  # the view itself is wanted as a gradient target (retain_grad(), a tensor hook on it): differentiate w.r.t. the view as the reference would -- it gets B equal
  # shares and autograd's ExpandBackward sums them.  (torch.autograd.grad(..., inputs=view) cannot be seen from here: pass the base, or a non-expanded tensor.)
  if t.retains_grad or t._backward_hooks: return t
  b = t._base
  if (b is not None and b.dim() == t.dim() and b.shape[0] == 1 and b.shape[1:] == t.shape[1:] and b.stride()[1:] == t.stride()[1:] and b.data_ptr() == t.data_ptr()
      and b.dtype is t.dtype and b.requires_grad == t.requires_grad):
    if '_dgp_hw' in t.__dict__: b.__dict__.setdefault('_dgp_hw', t.__dict__['_dgp_hw'])      # (a tiled grid's logical size travels with it)
    return b
  return t


def _check_versions(tensors, versions):
  """What autograd does when a SavedVariable is unpacked: a tensor the backward reads must not have been modified in place since the forward."""
  for t, v in zip(tensors, versions):
    if t is not None and t._version != v:
      raise RuntimeError('one of the variables needed for gradient computation has been modified by an inplace operation: a %s tensor '
                         'is at version %d; expected version %d (dgpmp2_amd PlanLayer backward)' % (list(t.shape), t._version, v))


def _grad_like(ref, like):
  """Uninitialised gradient buffer for input `ref`, written by the kernel as a contiguous array of the launch dtype (that of `like`):
  in ref's own shape when ref is contiguous and of that dtype (no reshape / cast afterwards), flat otherwise (see _grad_out)."""
  if ref.dtype is like.dtype and ref.is_contiguous():
    return torch.empty_like(ref)
  return like.new_empty((ref.numel(),))


def _grad_out(g, ref):
  if g is None or g.shape == ref.shape: return g
  g = g.reshape(ref.shape)
  return g if g.dtype is ref.dtype else g.to(ref.dtype)


class _SdfGrad(object):
  """Destination of dL/d(sdfb) for one backward launch, and its way back into autograd.

  shared grid (sdfb expand()ed / a single grid): `_SDF_GRAD_COPIES` PARTIAL grids, one set per XCD (XCD-local atomics), in FLOAT64 whatever the I/O type
      (DGP_GSDF_DENSE_F64): the sum over thousands of trajectories is formed in double and cast once, so the fp32 result no longer depends on the order in
      which the atomics landed; summed over the copies here.
  per-sample grids (the reference's API shape, sdfb (B,1,H,W) with `sdf_b.requires_grad_(True)`, learning/train_planner.py:267): the reference's gradient is a
      dense (B,1,H,W) tensor -- 1 GiB of zeros around 4 MB of taps at B = 4096, 256 x 256.  `layer.sdf_grad`:
        'dense'  (default) that tensor (zero-filled here, atomics in the kernel; the reference's layout);
        'sparse' a torch.sparse_coo_tensor of sdfb's shape holding the 4 n B taps (DGP_GSDF_SPARSE: no zero fill, no atomics; uncoalesced -- explicit zeros and
                 the duplicates of neighbouring states included; .to_dense() / .coalesce() give the reference's tensor).  AccumulateGrad takes a sparse gradient
                 for a dense leaf (sdfb.grad is then sparse, and sums with dense or sparse gradients from other nodes);
        'auto'   sparse when sdfb is a LEAF tensor, the trajectory has at most 256 states and the dense gradient would be larger than both
                 _SPARSE_MIN_DENSE_BYTES and twice the sparse one; dense otherwise (a non-leaf's producer may not accept sparse gradients).
  A tiled grid tensor (B,1,H/4,W/4,4,4) gets a gradient of its own shape either way: dense tiles, or a sparse tensor with six index rows."""

  __slots__ = ('g', 'idx', 'ptr', 'stride', 'copies', 'mode', 'shared', 'shape', 'pc', 'dev')

  def __init__(self, layer, th, sdf, sd, passes=1, zero_fill=False):
    B, n = th.shape[0], th.shape[1]
    H, W = sd[1], sd[2]
    self.shared = sd[3] == 0
    self.idx = None
    self.pc, self.dev = layer._pc, th.get_device()
    tiled = sd[4] != _capi.DGP_SDF_ROWMAJOR
    # the grid of one gradient: (1, H, W), or the (1, Ht, Wt, 4, 4) tiles of a tiled sdfb (the gradient of a tiled tensor is tiled)
    gshape = (1, (H + 3) // 4, (W + 3) // 4, 4, 4) if tiled else (1, H, W)
    gelems = gshape[1] * gshape[2] * (16 if tiled else 1)
    if self.shared:
      # partial copies: one per XCD; a single grid (device-scope atomics) for a small batch, whose few thousand taps do not contend -- zero-filling and summing
      # eight 256 x 256 double grids costs more than such a backward kernel runs
      self.copies, self.stride = (_SDF_GRAD_COPIES if B * n >= 8192 else 1), 0
      self.mode = _capi.DGP_GSDF_DENSE_F64 if n <= 256 else _capi.DGP_GSDF_DENSE
      self.g = torch.zeros((self.copies,) + gshape, dtype=torch.float64 if self.mode == _capi.DGP_GSDF_DENSE_F64 else th.dtype, device=th.device)
    else:
      self.copies, self.stride = 1, gelems
      want = layer.sdf_grad
      nnz = passes * B * n * 4
      sparse = False
      if want != 'dense' and n <= 256:
        dense_bytes, sparse_bytes = B * gelems * th.element_size(), nnz * ((48 if tiled else 32) + th.element_size())
        sparse = want == 'sparse' or (sdf.is_leaf and dense_bytes > _SPARSE_MIN_DENSE_BYTES and dense_bytes > 2 * sparse_bytes)
      if sparse:
        self.mode = _capi.DGP_GSDF_SPARSE
        mk = torch.zeros if zero_fill else torch.empty
        self.g = mk((nnz,), dtype=th.dtype, device=th.device)
        self.idx = mk((6 if tiled else 4, nnz), dtype=torch.int64, device=th.device)      # (b, 0, y, x), or the six indices of a tiled tensor (b, 0, y/4, x/4, y%4, x%4)
        self.shape = (B,) + tuple(sdf.shape[1:])
      else:
        self.mode = _capi.DGP_GSDF_DENSE
        self.g = th.new_zeros((B,) + gshape)
    self.ptr = self.g.data_ptr()

  def sd(self, sd):
    """The seven DgpSdf fields of the launch: the grid as marshalled for the forward + how its gradient is delivered."""
    return sd[:5] + (self.mode, None if self.idx is None else self.idx.data_ptr())

  def finish(self, sdf):
    """The launch's output -> the gradient in the layout autograd expects for `sdf`."""
    g = self.g
    if self.mode == _capi.DGP_GSDF_SPARSE:
      if g.dtype is not sdf.dtype: g = g.to(sdf.dtype)
      return torch.sparse_coo_tensor(self.idx, g, self.shape, check_invariants=False)      # (channel index 0: only channel 0 is read, obstacle_cost.py:35)
    if self.shared:
      # the copies summed (in double), scaled and cast in one launch; an expand()ed sdfb gets B equal shares: the kernel already accumulated all B
      # trajectories into the one grid, and autograd's expand-backward will sum the B slices of whatever is returned here
      many = sdf.shape[0] != 1
      out = torch.empty((1,) + tuple(g.shape[1:]), dtype=sdf.dtype if sdf.dtype in (torch.float32, torch.float64) else g.dtype, device=g.device)
      _launch(self.dev, self.pc.sum_partial_grids, g.data_ptr(), _io_code(g.dtype), self.copies, g[0].numel(), 1.0 / sdf.shape[0] if many else 1.0,
              out.data_ptr(), _io_code(out.dtype), _raw_stream(self.dev))
      g = out
      if sdf.shape[1] != 1:
        full = g.new_zeros((1,) + tuple(sdf.shape[1:]))
        full[:, 0:1] = g
        g = full
      if many: g = g.expand(sdf.shape)
      return g if g.dtype is sdf.dtype else g.to(sdf.dtype)
    if sdf.shape[1] != 1:       # only channel 0 is read (obstacle_cost.py:35): the other channels get a zero gradient
      full = g.new_zeros((g.shape[0],) + tuple(sdf.shape[1:]))
      full[:, 0:1] = g
      g = full
    return g if g.dtype is sdf.dtype else g.to(sdf.dtype)


class _NoSdfGrad(object):
  ptr, stride, copies = None, 0, 1

  @staticmethod
  def sd(sd): return sd[:7]

  @staticmethod
  def finish(sdf): return None


_NO_SDF_GRAD = _NoSdfGrad()
_SPARSE_MIN_DENSE_BYTES = 16 << 20      # 'auto': below this a zero-filled dense gradient costs a few microseconds and keeps the reference's layout


def _diff_needs(ctx, slots, first, count):
  """Which of a node's `count` inputs ts[i] need a gradient: only diff = [ts[i] for i in slots] are ARGUMENTS of the Function, from position `first` on."""
  nig = ctx.needs_input_grad
  need = [False] * count
  for q, i in enumerate(slots): need[i] = nig[first + q]
  return need


def _cot(g, dtype):
  """A cotangent as a launch reads it: of the launch dtype and contiguous (an unused output's stays None)."""
  return g if (g is None or (g.dtype is dtype and g.is_contiguous())) else g.contiguous().to(dtype)


def _versions(*ts):
  return tuple([-1 if t is None else t._version for t in ts])


def _backward_of(impl):
  """The `backward` staticmethod of a node whose backward is a raw kernel: a double backward must raise instead of silently returning zeros.  torch's
  once_differentiable does that, at ~8 us of wrapper per call; grad mode is only enabled inside backward() under create_graph=True, so the wrapper
  is only paid there."""
  once = once_differentiable(impl)

  def backward(ctx, *cots):
    if torch.is_grad_enabled():
      return once(ctx, *cots)
    return impl(ctx, *cots)
  return staticmethod(backward)


def _keep_step(ctx, layer, slots, r, sdf, covs, start, goal):
  """What the backward of a step node needs of its forward launch `r` (_GNStep.launch's tuple); covs = the covariance inputs behind the grid in `ts`."""
  thc, stc, goc = r[6]
  ctx.layer, ctx.slots = layer, slots
  ctx.args = r[7]                               # marshalled SDF / covariance arguments (and the converted copies they point into)
  # Inputs: the backward needs their ADDRESSES (in ctx.args) and, for the gradient buffers, their shapes -- not SavedVariables, whose
  # unpacking costs ~1.5 us per tensor.  What save_for_backward would add, the "modified by an inplace operation" check, is done
  # by hand on the version counters.  (dth is an OUTPUT: it must go through save_for_backward, a plain reference would be a cycle.)
  ctx.inputs = (thc, stc, goc, sdf) + covs + (start, goal)
  ctx.versions = _versions(thc, stc, goc, sdf, *covs)
  ctx.save_for_backward(r[0])
  ctx.set_materialize_grads(False)              # an unused output arrives as None: no adjoint solve for an err_ext-only loss


def _step_backward(ctx, need, g_dth, g_eex, g_err, g_covs):
  """The backward launch of a step node: dgp_gn_step_backward, or -- g_err = the cotangents of the three unweighted errors, not None -- dgp_gn_step_errors_backward.
  need[0:4]: which of th, start, goal, sdf get a gradient; g_covs: the three covariance-gradient buffers (or None), the caller's.  -> (g_th, g_start, g_goal, the _SdfGrad to finish() into g_sdf: the raw node's covariance launch goes first)"""
  layer = ctx.layer
  dth, = ctx.saved_tensors
  _check_versions(ctx.inputs, ctx.versions)
  th, stc, goc, sdf = ctx.inputs[:4]
  start, goal = ctx.inputs[-2:]
  sd, cv = ctx.args
  B, n, d = th.shape
  dtype = th.dtype
  solver = layer._solvers[dtype]
  dev = th.get_device()
  g_dth, g_eex = _cot(g_dth, dtype), _cot(g_eex, dtype)
  g_th = torch.empty_like(th) if need[0] else None
  g_st = _grad_like(start, stc) if need[1] else None
  g_go = _grad_like(goal, goc) if need[2] else None
  g_qc, g_ow, g_eps = g_covs
  if g_err is None:
    gs = _SdfGrad(layer, th, sdf, sd) if need[3] else _NO_SDF_GRAD
    _launch(dev, layer._pc.gn_step_backward, solver.h, B, th.data_ptr(), stc.data_ptr(), goc.data_ptr(), *gs.sd(sd),
            *cv[:4], dth.data_ptr(), _ptr(g_dth), _ptr(g_eex), _ptr(g_th), _ptr(g_st), _ptr(g_go), gs.ptr, gs.stride, gs.copies,
            _ptr(g_qc), _ptr(g_ow), _ptr(g_eps), _raw_stream(dev))
  else:
    g_usg, g_ugp, g_uobs = _cot(g_err[0], dtype), _cot(g_err[1], dtype), _cot(g_err[2], dtype)
    errs = g_usg is not None or g_ugp is not None or g_uobs is not None
    gs = _SdfGrad(layer, th, sdf, sd, passes=2 if errs else 1) if need[3] else _NO_SDF_GRAD      # (with error cotangents the grid is read at th + dtheta and at th)
    # d = 4: the errors' backward runs as a prologue of the step's backward kernel (one launch, hand-over in LDS); the two-launch form of the (x, y, theta)
    # robot and of long trajectories hands dL/d(th + dtheta) over in a workspace
    ws = torch.empty_like(th) if (errs and (d != 4 or n > 256)) else None
    _launch(dev, layer._pc.gn_step_errors_backward, solver.h, B, th.data_ptr(), stc.data_ptr(), goc.data_ptr(), *gs.sd(sd),
            *cv[:4], dth.data_ptr(), _ptr(g_dth), _ptr(g_eex), _ptr(g_usg), _ptr(g_ugp), _ptr(g_uobs), _ptr(g_th), _ptr(g_st),
            _ptr(g_go), gs.ptr, gs.stride, gs.copies, _ptr(g_qc), _ptr(g_ow), _ptr(g_eps), _ptr(ws), _raw_stream(dev))
  return g_th, _grad_out(g_st, start), _grad_out(g_go, goal), gs


def _covs_step_forward(ctx, with_errors, layer, static, slots, ts, box):
  """forward of _GNStep / _GNStepErrors -> the launch's tuple.  ts = (th, start, goal, sdf, qc, ow, eps), every input; diff = those of them that require grad,
  ts[i] for i in slots.  Only `diff` are tensor ARGUMENTS of the Function (the bookkeeping of Function.apply is paid per tensor argument: ~1 us each, and a TBPTT link
  differentiates one of the seven); err -- never differentiable, plan_layer.py:275 -- leaves through `box` instead of as an output."""
  th, start, goal, sdf, qc, ow, eps = ts
  r = _GNStep.launch(layer, with_errors, static, th, start, goal, sdf, qc, ow, eps, True)
  box.append(r[1])
  _keep_step(ctx, layer, slots, r, sdf, (qc, ow, eps), start, goal)
  return r


def _covs_step_backward(ctx, g_dth, g_eex, g_err):
  """backward of _GNStep / _GNStepErrors: the gradient buffers of the covariance tensors the launch streamed, the shared launch, the gradients of `diff`."""
  slots = ctx.slots
  need = _diff_needs(ctx, slots, 5, 7)            # (layer, static, slots, ts, box, *diff)
  th, qc, ow, eps = ctx.inputs[0], ctx.inputs[4], ctx.inputs[5], ctx.inputs[6]
  cv = ctx.args[1]
  g_qc = _grad_like(qc, th) if (need[4] and cv[1] is not None) else None
  g_ow = _grad_like(ow, th) if (need[5] and cv[2] is not None) else None
  g_eps = _grad_like(eps, th) if (need[6] and cv[3] is not None) else None
  g_th, g_st, g_go, gs = _step_backward(ctx, need, g_dth, g_eex, g_err, (g_qc, g_ow, g_eps))
  grads = (g_th, g_st, g_go, gs.finish(ctx.inputs[3]), _grad_out(g_qc, qc), _grad_out(g_ow, ow), _grad_out(g_eps, eps))
  return (None, None, None, None, None) + tuple(grads[i] for i in slots)


class _GNStep(torch.autograd.Function):
  """dtheta, err, err_ext = GN step; backward through dgp_gn_step_backward (adjoint block-tridiagonal solve)."""

  @staticmethod
  def launch(layer, with_errors, static, th, start, goal, sdf, qc, ow, eps, own_info=False):
    """The forward launch itself (no autograd bookkeeping): dgp_gn_step, or -- with_errors -- dgp_gn_step_errors, which also writes the three unweighted errors
    at th + dtheta.  -> dth, err, eex, usg, ugp, uobs (the last three None without errors), and what the backward needs: the contiguous inputs, the marshalled
    SDF / covariance arguments with the tensors they keep alive."""
    B = th.shape[0]
    dtype = th.dtype
    solver = layer._solvers.get(dtype) or layer._solver(dtype)
    dev = th.get_device()
    if start.get_device() != dev or goal.get_device() != dev:
      _same_device(dev, startb=start, goalb=goal)
    sd = layer._sdf_args(sdf, dtype, B, dev)
    if static.__class__ is _RawCovs: cv = static.cov_args(B, dtype, dev)      # (qc is the learn module's raw output vector, squared inside the kernel)
    else: cv = _NO_COVS_KEEP if static == _ALL_STATIC else layer._cov_args(qc, ow, eps, dtype, B, dev, static, True)
    thc, stc, goc = th.contiguous(), start.contiguous(), goal.contiguous()
    dth = torch.empty_like(thc)
    proto = layer._err_protos.get((B, dtype, dev))
    if proto is None: proto = layer._err_proto(B, dtype, dev, thc)
    err = torch.empty_like(proto)           # (empty_like of a cached (B,1,1) tensor: 1.3 us; new_empty / torch.empty with a shape: 2.1 us)
    eex = torch.empty_like(proto)
    stream = _raw_stream(dev)
    # SPD flags: a differentiable step (own_info) or a checking layer gets its own tensor -- `last_info` kept from iteration k stays that
    # iteration's; the planning loop without an autograd graph reuses one buffer per (batch, device, stream), see _info_buffer
    info = layer._info_buffer(B, dev, stream, thc)
    if own_info or layer.check_spd: info = torch.empty_like(info)
    if with_errors:
      usg, ugp, uobs = torch.empty_like(proto), torch.empty_like(proto), torch.empty_like(proto)
      _launch(dev, layer._pc.gn_step_errors, solver.h, B, thc.data_ptr(), stc.data_ptr(), goc.data_ptr(), *sd[:7], *cv[:4], dth.data_ptr(), err.data_ptr(), eex.data_ptr(), info.data_ptr(),
              usg.data_ptr(), ugp.data_ptr(), uobs.data_ptr(), stream)
    else:
      usg = ugp = uobs = None
      _launch(dev, layer._pc.gn_step, solver.h, B, thc.data_ptr(), stc.data_ptr(), goc.data_ptr(), *sd[:7], *cv[:4], dth.data_ptr(), err.data_ptr(), eex.data_ptr(), info.data_ptr(), stream)
    layer.__dict__['last_info'] = info      # (plain attribute: nn.Module.__setattr__ costs microseconds per call)
    if layer.check_spd and bool(info.any()):
      raise RuntimeError('dgpmp2_amd: A^T K A + delta I is not positive definite for %d of %d trajectories '
                         '(the reference raises from torch.cholesky here)' % (int(info.sum()), B))
    return dth, err, eex, usg, ugp, uobs, (thc, stc, goc), (sd, cv)

  @staticmethod
  def forward(ctx, layer, static, slots, ts, box, *diff):
    r = _covs_step_forward(ctx, False, layer, static, slots, ts, box)
    return r[0], r[2]

  def _impl(ctx, g_dth, g_eex):
    return _covs_step_backward(ctx, g_dth, g_eex, None)

  backward = _backward_of(_impl)


class _GNStepErrors(torch.autograd.Function):
  """One iteration of the reference's training loop as ONE autograd node (learning/train_planner.py:311-327): dtheta, err, err_ext of the
  step AND the three unweighted errors at th + dtheta -- forward = dgp_gn_step_errors, backward = dgp_gn_step_errors_backward (one
  launch each for the 2-D robot with a row-major grid and up to 128 / 256 states, two stream-ordered launches otherwise, behind one C-ABI call; no th + dtheta tensor,
  no second Function.apply, no second trip through the autograd engine)."""

  @staticmethod
  def forward(ctx, layer, static, slots, ts, box, *diff):
    r = _covs_step_forward(ctx, True, layer, static, slots, ts, box)
    return r[0], r[2], r[3], r[4], r[5]

  def _impl(ctx, g_dth, g_eex, g_usg, g_ugp, g_uobs):
    return _covs_step_backward(ctx, g_dth, g_eex, (g_usg, g_ugp, g_uobs))

  backward = _backward_of(_impl)


class _RawCovs(object):
  """The learn module's output vector as the covariance input of a step: `out` (B, 1, W) contiguous, column blocks [0, n_gp) one raw scalar q_k per GP factor
  ('diag_identity': Q_c^-1 = q_k^2 I; n_gp = 0: 'fix_dynamics', the static Q_c_inv), [n_gp, n_gp + n) the raw obstacle weights o_i (weight o_i^2), then --
  learn_eps -- the raw epsilons (eps = e_i^2): exactly what get_covariances slices and squares for a single-link robot (diff_gpmp2_planner.py:247-290).  ONE small
  launch (dgp_square_covariances) forms every tensor the step and its caller need -- the scalars q_k^2 the kernels take (DGP_QC_SCALAR), the blocks q_k^2 I the
  reference returns, o_i^2, e_i^2 -- and one more (dgp_square_covariances_backward) turns the gradients the backward kernel writes into d/d out."""

  __slots__ = ('out', 'n_gp', 'n', 'learn_eps', 'dof', 'scal', 'qc', 'ow', 'eps')

  def __init__(self, out, n_gp, n, learn_eps, dof):
    self.out, self.n_gp, self.n, self.learn_eps, self.dof = out, n_gp, n, learn_eps, dof
    self.scal = self.qc = self.ow = self.eps = None

  @property
  def used(self): return self.n_gp + self.n * (2 if self.learn_eps else 1)

  def square(self, pc, dev):
    """the forward launch: fills scal (B, n-1), qc (B, n-1, dof, dof), ow (B, n, 1, 1), eps (B, n, 1, 1) (those the mode has)"""
    out = self.out
    B, n = out.shape[0], self.n
    if self.n_gp:
      self.scal = out.new_empty((B, self.n_gp))
      self.qc = out.new_empty((B, self.n_gp, self.dof, self.dof))
    self.ow = out.new_empty((B, n, 1, 1))
    if self.learn_eps: self.eps = out.new_empty((B, n, 1, 1))
    _launch(dev, pc.square_covariances, out.data_ptr(), _io_code(out.dtype), B, out.shape[2], self.n_gp, n, int(self.learn_eps), self.dof, _ptr(self.scal), _ptr(self.qc),
            self.ow.data_ptr(), _ptr(self.eps), _raw_stream(dev))

  def cov_args(self, B, dtype, dev):
    return (_capi.DGP_QC_SCALAR if self.n_gp else _capi.DGP_QC_STATIC, _ptr(self.scal), self.ow.data_ptr(), _ptr(self.eps), (self.scal, self.ow, self.eps))


class _GNStepRaw(torch.autograd.Function):
  """_GNStep / _GNStepErrors with the learn module's OUTPUT VECTOR as the covariance input (planner.step() / step_with_errors() in the learned modes
  'diag_identity' and 'fix_dynamics' of a single-link robot): the squares of diff_gpmp2_planner.py:247-290 are taken inside the kernels and the backward kernel
  writes dL/d out -- none of get_covariances' slices, products and their backward (a dozen small torch kernels that cost as much as the solver under HIP-graph
  replay) is left.  Outputs: dtheta, err_ext[, the three unweighted errors at th + dtheta], and the squared tensors step() returns (differentiable: a cotangent
  on them, which the reference's loss does not produce -- its cov_loss is commented out, learning/train_planner.py:115 -- is chained by plain torch ops)."""

  @staticmethod
  def forward(ctx, layer, raw, with_errors, slots, ts, box, *diff):
    th, start, goal, sdf, out = ts
    raw.square(layer._pc, th.get_device())
    r = _GNStep.launch(layer, with_errors, raw, th, start, goal, sdf, out, None, None, True)
    # (aliases as outputs: the node keeps raw.scal / ow / eps for its backward launch, and an OUTPUT held by its own node would be a reference cycle)
    qc, ow, eps = (None if t is None else t.view(t.shape) for t in (raw.qc, raw.ow, raw.eps))
    box.append((r[1],))
    _keep_step(ctx, layer, slots, r, sdf, (out,), start, goal)
    ctx.raw, ctx.with_errors = raw, with_errors
    return (r[0], r[2]) + (r[3:6] if with_errors else ()) + tuple(t for t in (qc, ow, eps) if t is not None)

  def _impl(ctx, *cots):
    layer, raw, slots = ctx.layer, ctx.raw, ctx.slots
    out = ctx.inputs[4]
    need = _diff_needs(ctx, slots, 6, 5)          # (layer, raw, with_errors, slots, ts, box, *diff)
    k = 5 if ctx.with_errors else 2
    g_out = gq = gw = ge = None
    if need[4]:
      # the backward kernel writes the gradients of the squared tensors (the blocks' gradient under DGP_QC_SCALAR); one more small launch turns them into d/d out
      if raw.n_gp: gq = torch.empty_like(raw.qc)
      gw = torch.empty_like(raw.ow)
      if raw.learn_eps: ge = torch.empty_like(raw.eps)
    g_th, g_st, g_go, gs = _step_backward(ctx, need, cots[0], cots[1], cots[2:5] if ctx.with_errors else None, (gq, gw, ge))
    if need[4]:
      # someone differentiated the squared tensors themselves (the reference's loss does not): their cotangents (qc [if n_gp], ow, eps [if learn_eps]: normally
      # all None) join the kernel's gradients
      dtype, dev = out.dtype, out.get_device()
      names = (['qc'] if raw.n_gp else []) + ['ow'] + (['eps'] if raw.learn_eps else [])
      for name, g in zip(names, cots[k:]):
        if g is None: continue
        if name == 'qc': gq = gq + g.to(dtype)
        elif name == 'ow': gw = gw + g.reshape(gw.shape).to(dtype)
        else: ge = ge + g.reshape(ge.shape).to(dtype)
      g_out = torch.empty_like(out)
      _launch(dev, layer._pc.square_covariances_backward, out.data_ptr(), _io_code(dtype), out.shape[0], out.shape[2], raw.n_gp, raw.n, int(raw.learn_eps), raw.dof,
              _ptr(gq), _ptr(gw), _ptr(ge), g_out.data_ptr(), _raw_stream(dev))
    grads = (g_th, g_st, g_go, gs.finish(ctx.inputs[3]), g_out)
    return (None, None, None, None, None, None) + tuple(grads[i] for i in slots)

  backward = _backward_of(_impl)


class _GNSolve(torch.autograd.Function):
  """The whole Gauss-Newton loop of DiffGPMP2Planner.forward as ONE autograd node: forward = dgp_gn_solve_traced (the fused loop, keeping the
  fp64 history of the trajectory), backward = dgp_gn_solve_backward (one launch that walks the iterations backwards per trajectory).  The
  reference keeps the graph across its python loop (diff_gpmp2_planner.py:122-156); K iterations there are K x (dense solve + 2 error
  evaluations) nodes, here two launches whatever K is."""

  @staticmethod
  def forward(ctx, layer, max_iters, tol_delta, slots, ts, box, *diff):
    """ts = (th_init, start, goal, sdf); box receives (iters, err_hist, errext_hist, err_final, info) -- none of them differentiable
    (forward() returns the errors as python floats, :138-141,162-164)."""
    th, start, goal, sdf = ts
    B, n, d = th.shape
    dtype = th.dtype
    solver = layer._solvers.get(dtype) or layer._solver(dtype)
    dev = th.get_device()
    sd = layer._sdf_args(sdf, dtype, B, dev)
    thc, stc, goc = th.contiguous(), start.contiguous(), goal.contiguous()
    th_out = torch.empty_like(thc)
    m = max_iters
    buf = torch.full((B * (2 * m + 3),), float('nan'), dtype=dtype, device=th.device)      # err history | err_ext history | final error | iteration counts | SPD flags: one copy to the host
    eh, eeh, ef = buf[:B * m], buf[B * m:2 * B * m], buf[2 * B * m:2 * B * m + B]
    iters = buf[2 * B * m + B:].view(torch.int32)[:B]
    info = buf[2 * B * m + 2 * B:].view(torch.int32)[:B]
    hist = torch.empty((m, B, n, d), dtype=torch.float64, device=th.device)      # th_k, fp64 whatever the I/O type (rows past iters[b] stay unwritten and unread)
    _launch(dev, layer._pc.gn_solve_traced, solver.h, B, thc.data_ptr(), stc.data_ptr(), goc.data_ptr(), *sd[:7], *_NO_COVS,
            max_iters, tol_delta, th_out.data_ptr(), iters.data_ptr(), eh.data_ptr(), eeh.data_ptr(), ef.data_ptr(), info.data_ptr(), hist.data_ptr(),
            _raw_stream(dev))
    box.append((buf, info))
    ctx.layer, ctx.slots, ctx.max_iters = layer, slots, max_iters
    ctx.args = sd
    ctx.inputs = (stc, goc, sdf, start, goal, thc)
    ctx.versions = _versions(stc, goc, sdf)
    ctx.hist, ctx.iters = hist, iters               # (work buffers of this node, never handed out: plain references)
    ctx.save_for_backward(th_out)
    return th_out

  @staticmethod
  @once_differentiable
  def backward(ctx, g_out):
    layer = ctx.layer
    th_out, = ctx.saved_tensors
    stc, goc, sdf, start, goal, thc = ctx.inputs
    _check_versions(ctx.inputs[:3], ctx.versions)
    sd = ctx.args
    B, n, d = th_out.shape
    dtype = th_out.dtype
    solver = layer._solvers[dtype]
    dev = th_out.get_device()
    need = _diff_needs(ctx, ctx.slots, 6, 4)      # (layer, max_iters, tol_delta, slots, ts, box, *diff)
    g_out = _cot(g_out, dtype)
    g_th = torch.empty_like(th_out) if need[0] else None
    g_st = _grad_like(start, stc) if need[1] else None
    g_go = _grad_like(goal, goc) if need[2] else None
    gs = _SdfGrad(layer, th_out, sdf, sd, passes=ctx.max_iters, zero_fill=True) if need[3] else _NO_SDF_GRAD      # (a trajectory writes only the passes it ran)
    _launch(dev, layer._pc.gn_solve_backward, solver.h, B, stc.data_ptr(), goc.data_ptr(), *gs.sd(sd), ctx.max_iters,
            ctx.hist.data_ptr(), th_out.data_ptr(), ctx.iters.data_ptr(), g_out.data_ptr(), _ptr(g_th), _ptr(g_st), _ptr(g_go), gs.ptr, gs.stride,
            gs.copies, _raw_stream(dev))
    g_sdf = gs.finish(sdf)
    grads = (g_th, _grad_out(g_st, start), _grad_out(g_go, goal), g_sdf)
    return (None, None, None, None, None, None) + tuple(grads[i] for i in ctx.slots)


_NO_COVS_KEEP = _NO_COVS + ((),)


class _EvalErrors(torch.autograd.Function):
  """err_ext, start_goal_error, gp_error, obs_error at a trajectory = one launch of dgp_eval_errors; backward = one launch of
  dgp_eval_errors_backward.  These are the quantities the reference's training loss differentiates besides dtheta
  (learning/train_planner.py:327,342 -> one_step_loss :75-120): plain torch ops there (plan_layer.py:310-345, :374-388), hence
  differentiable w.r.t. thb, sdfb, the start / goal means and the current eps (all remembered WITH their graphs by the last
  forward(), plan_layer.py:88-94).  None of them depends on qc_inv / obscov_inv (fixed or unit weights)."""

  @staticmethod
  def forward(ctx, layer, slots, ts, *diff):
    """ts = (th, start, goal, sdf, eps); diff = ts[i] for i in slots, the inputs that require grad (see _covs_step_forward)."""
    th, start, goal, sdf, eps = ts
    eps_arg = None if (eps is None or '_dgp_static' in eps.__dict__) else eps
    o, thc, stc, goc, sd, cv = layer._eval_launch(th, sdf, start, goal, None, None, eps_arg)
    ctx.layer = layer
    ctx.slots = slots
    ctx.args = (sd, cv)
    ctx.inputs = (thc, stc, goc, sdf, eps_arg, start, goal)      # (addresses in ctx.args; version counters checked by hand, see _covs_step_forward)
    ctx.versions = _versions(thc, stc, goc, sdf, eps_arg)
    ctx.set_materialize_grads(False)
    return o[1], o[2], o[3], o[4]            # (the three that read the grid are None without one)

  def _impl(ctx, g_eex, g_usg, g_ugp, g_uobs):
    layer = ctx.layer
    th, stc, goc, sdf, eps, start, goal = ctx.inputs
    _check_versions(ctx.inputs, ctx.versions)
    sd, cv = ctx.args
    B, n, d = th.shape
    dtype = th.dtype
    solver = layer._solvers[dtype]
    dev = th.get_device()
    need = _diff_needs(ctx, ctx.slots, 3, 5)          # (layer, slots, ts, *diff)
    cot = [_cot(g, dtype) for g in (g_eex, g_usg, g_ugp, g_uobs)]
    g_th = torch.empty_like(th) if need[0] else None
    g_st = _grad_like(start, stc) if need[1] else None
    g_go = _grad_like(goal, goc) if need[2] else None
    gs = _SdfGrad(layer, th, sdf, sd) if (sdf is not None and need[3]) else _NO_SDF_GRAD
    g_eps = _grad_like(eps, th) if (need[4] and eps is not None) else None
    _launch(dev, layer._pc.eval_errors_backward, solver.h, B, th.data_ptr(), stc.data_ptr(), goc.data_ptr(), *gs.sd(sd),
            *cv[:4], _ptr(cot[0]), _ptr(cot[1]), _ptr(cot[2]), _ptr(cot[3]), _ptr(g_th), _ptr(g_st), _ptr(g_go), gs.ptr,
            gs.stride, gs.copies, _ptr(g_eps), _raw_stream(dev))
    g_sdf = gs.finish(sdf)
    grads = (g_th, _grad_out(g_st, start), _grad_out(g_go, goal), g_sdf, _grad_out(g_eps, eps))
    return (None, None, None) + tuple(grads[i] for i in ctx.slots)

  backward = _backward_of(_impl)


class _AutoTile(torch.autograd.Function):
  """PlanLayer.auto_tile: a per-sample ROW-MAJOR sdfb (B,1,H,W) stands in the graph, the kernels read its 4 x 4-tiled copy `tiles` (made once per batch of grids,
  PlanLayer._auto_tiled).  forward: the cached tiles, no work; backward: the gradient of the tiled tensor -> the gradient of the row-major one -- a dense tiled gradient
  is un-tiled (views + one slice: AccumulateGrad's copy is the only pass over it), a sparse one (six index rows b,0,y/4,x/4,y%4,x%4) gets the four row-major index
  rows (b,0,y,x); taps of padding cells do not exist (the lookup clamps to H-1 / W-1)."""

  @staticmethod
  def forward(ctx, sdfb, tiles):
    ctx.hw = (int(sdfb.shape[-2]), int(sdfb.shape[-1]))
    ctx.shape = tuple(sdfb.shape)
    return tiles.detach()

  @staticmethod
  @once_differentiable
  def backward(ctx, g):
    H, W = ctx.hw
    if g.is_sparse:
      i = g._indices()
      idx = torch.stack((i[0], i[1], i[2] * 4 + i[4], i[3] * 4 + i[5]))
      return torch.sparse_coo_tensor(idx, g._values(), ctx.shape, check_invariants=False), None
    with torch._C.DisableTorchFunctionSubclass():
      B, C_, Ht, Wt = g.shape[:4]
      return g.permute(0, 1, 2, 4, 3, 5).reshape(B, C_, Ht * 4, Wt * 4)[:, :, :H, :W], None


class LossTerms(collections.namedtuple('LossTerms', 'total pos vel cov gp sg obs ext')):
  """What device_step_loss returns: the eight terms of the reference's one_step_loss in its return order (learning/train_planner.py:120), 0-d float64 device tensors
  on the storage of the one (8,) result `.raw` (no slice or cast kernels) -- `total` is differentiable, the others carry no graph (the reference only ever .item()s them) -- and
  `.per_sample` (B, 5) float64: per trajectory the summed squared position and velocity miss (over states and columns) and the three errors (pos, vel, gp, sg, obs)."""
  raw = per_sample = None


def _loss_weights(weights):
  """(vel_loss_lambda, ext_obs_lambda, ext_loss_weight) as python floats from learn_params['optim'] (or any mapping with those keys)"""
  return _f(weights['vel_loss_lambda']), _f(weights['ext_obs_lambda']), _f(weights['ext_loss_weight'])


def _loss_in(t, dtype):
  """An input of the loss launches as they read it: of the launch dtype and contiguous"""
  return t if (t is None or (t.dtype is dtype and t.is_contiguous())) else t.to(dtype).contiguous()


class _StepLoss(torch.autograd.Function):
  """The loss of one training iteration as ONE autograd node: forward = dgp_step_loss (two stream-ordered launches), backward = ONE dgp_step_loss_backward launch
  that reads the incoming 0-d cotangent from device memory.  Outputs: total (differentiable), the (8,) terms and the (B, 5) per-trajectory array (not
  differentiable: the reference only ever .item()s the other terms)."""

  @staticmethod
  def forward(ctx, pc, w, dof, update, target, target_sub, e_sg, e_gp, e_obs):
    B, n, d = update.shape
    dtype, dev = update.dtype, update.get_device()
    u, t, s = update.contiguous(), _loss_in(target, dtype), _loss_in(target_sub, dtype)
    sg, gp, ob = _loss_in(e_sg, dtype), _loss_in(e_gp, dtype), _loss_in(e_obs, dtype)
    terms = torch.empty((_capi.DGP_LOSS_COUNT,), dtype=torch.float64, device=u.device)
    per = torch.empty((B, _capi.DGP_LOSS_PER_TRAJ), dtype=torch.float64, device=u.device)
    _launch(dev, pc.step_loss, _io_code(dtype), B, n, dof, u.data_ptr(), t.data_ptr(), _ptr(s), _ptr(sg), _ptr(gp), _ptr(ob), w[0], w[1], w[2], terms.data_ptr(),
            per.data_ptr(), _raw_stream(dev))
    ctx.pc, ctx.w, ctx.dof = pc, w, dof
    ctx.refs = (update, target, target_sub, e_sg, e_gp, e_obs)      # shapes and dtypes of the gradients to return (the launch reads the saved tensors)
    ctx.save_for_backward(u, t, s)
    ctx.mark_non_differentiable(terms, per)
    ctx.set_materialize_grads(False)
    return terms.new_empty(()).set_(terms.untyped_storage(), 0, ()), terms, per      # terms[0], as a tensor of its own: `terms` is handed out without a graph

  def _impl(ctx, g_total, _g_terms, _g_per):
    if g_total is None: return (None,) * 9
    u, t, s = ctx.saved_tensors
    update, target, target_sub, e_sg, e_gp, e_obs = ctx.refs
    need = ctx.needs_input_grad[3:]
    B, n, d = u.shape
    dtype, dev = u.dtype, u.get_device()
    g = g_total if (g_total.dtype is torch.float64 and g_total.is_contiguous()) else g_total.to(torch.float64).contiguous()
    g_u = torch.empty_like(u) if need[0] else None
    g_t = torch.empty_like(u) if need[1] else None
    g_s = torch.empty_like(u) if (need[2] and target_sub is not None) else None
    errs = [u.new_empty((B,)) if (nd and e is not None) else None for nd, e in zip(need[3:], (e_sg, e_gp, e_obs))]
    if g_u is None and g_t is None and g_s is None and errs == [None, None, None]: return (None,) * 9
    w = ctx.w
    _launch(dev, ctx.pc.step_loss_backward, _io_code(dtype), B, n, ctx.dof, u.data_ptr(), t.data_ptr(), _ptr(s), w[0], w[1], w[2], g.data_ptr(), _ptr(g_u), _ptr(g_t),
            _ptr(g_s), _ptr(errs[0]), _ptr(errs[1]), _ptr(errs[2]), _raw_stream(dev))
    back = lambda gr, ref: None if gr is None else _grad_out(gr, ref)
    return (None, None, None, back(g_u, update), back(g_t, target), back(g_s, target_sub), back(errs[0], e_sg), back(errs[1], e_gp), back(errs[2], e_obs))

  backward = _backward_of(_impl)


def device_step_loss(pc, dof, update, target, target_sub, errors, weights):
  """dgp_step_loss on device tensors -> LossTerms.  update, target (B,n,d) and target_sub (B,n,d) or None: the per-element miss is update - (target - target_sub);
  errors = (err_sg, err_gp, err_obs), each with B elements or None (a zero term); weights: a mapping with 'vel_loss_lambda', 'ext_obs_lambda', 'ext_loss_weight'.
  Positions are columns [0, dof), velocities [dof, 2 dof) (the reference hard-codes columns 0,1 / 2,3: the same for dof 2).  The tensors take update's dtype."""
  if dof not in (2, 3): raise ValueError('dof must be 2 or 3, got %r' % (dof,))
  if update.dim() != 3 or update.shape[2] != 2 * dof: raise ValueError('update must be (B,n,%d), got %s' % (2 * dof, tuple(update.shape)))
  if update.dtype not in (torch.float32, torch.float64): raise TypeError('dgpmp2_amd supports float32 and float64 tensors, got %s' % update.dtype)
  dev = update.get_device()
  if dev < 0: _require_cuda(update, 'update')
  B = update.shape[0]
  if target is None: raise ValueError('target is required')
  for name, t in (('target', target), ('target_sub', target_sub)):
    if t is not None and t.shape != update.shape: raise ValueError('%s must have the shape of update %s, got %s' % (name, tuple(update.shape), tuple(t.shape)))
  errors = tuple(errors) + (None,) * (3 - len(errors))
  for name, e in zip(('err_sg', 'err_gp', 'err_obs'), errors):
    if e is not None and e.numel() != B: raise ValueError('%s must hold one value per trajectory (%d), got %s' % (name, B, tuple(e.shape)))
  _same_device(dev, target=target, target_sub=target_sub, err_sg=errors[0], err_gp=errors[1], err_obs=errors[2])
  total, terms, per = _StepLoss.apply(pc, _loss_weights(weights), dof, update, target, target_sub, *errors)
  out = LossTerms(total, *terms.unbind(0)[1:])
  out.raw, out.per_sample = terms, per
  return out


class PlanLayer(nn.Module):
  """See module docstring.  Constructor mirrors plan_layer.py:14."""

  def __init__(self, gp_params, obs_params, planner_params, optim_params, env_params, robot_model, learn_params=None, batch_size=1,
               use_cuda=False, check_spd=False):
    super(PlanLayer, self).__init__()
    self.use_cuda = torch.cuda.is_available() if use_cuda else False
    self.device = torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')
    self.gp_params, self.obs_params, self.planner_params = gp_params, obs_params, planner_params
    self.optim_params, self.env_params, self.robot_model, self.learn_params = optim_params, env_params, robot_model, learn_params
    self.batch_size = batch_size
    self.dof = int(planner_params['dof'])
    self.state_dim = int(planner_params['state_dim'])
    if self.state_dim != 2 * self.dof:
      raise ValueError('state_dim must be 2*dof (position + velocity)')
    self.total_time_sec = planner_params['total_time_sec']
    self.total_time_step = int(planner_params['total_time_step'])
    self.num_traj_states = self.total_time_step + 1
    self.dt = self.total_time_sec * 1.0 / self.total_time_step * 1.0
    self.non_holonomic = bool(planner_params['non_holonomic']) if 'non_holonomic' in planner_params else False
    self.use_vel_limits = bool(planner_params['use_vel_limits']) if 'use_vel_limits' in planner_params else False
    self.num_gp_factors = self.num_traj_states - 1
    self.num_prior_factors = 2
    self.num_obs_factors = self.num_traj_states
    self.nlinks = robot_model.nlinks
    self.M = self.state_dim * (self.num_gp_factors + self.num_prior_factors) + self.num_obs_factors * self.nlinks
    if self.non_holonomic: self.M = self.M + self.num_traj_states
    if self.use_vel_limits: self.M = self.M + self.dof * self.num_traj_states
    self.N = self.state_dim * self.num_traj_states
    self.dynamics_mode = learn_params['dgpmp2']['dynamics_mode'] if learn_params is not None else None
    self._q_full = learn_params is not None and self.dynamics_mode == 'q_full'        # plan_layer.py:90
    self.check_spd = check_spd
    # how the gradient of PER-SAMPLE grids is returned: 'dense' (default: the reference's layout, a dense tensor of sdfb's shape) | 'sparse' | 'auto' (sparse for
    # large leaf grids) -- see _SdfGrad; sparse gradients are an opt-in because optimisers, clip_grad_norm_ and DDP buckets do not take them
    self.sdf_grad = 'dense'
    self.sdf_hw = None                 # logical (H, W) of tiled grids that arrive as PLAIN (B,1,Ht,Wt,4,4) tensors (a utils.sdf_utils.TiledSdf carries its own)
    # True: a per-sample row-major sdfb (B,1,H,W) -- the reference's API shape -- is tiled ONCE per batch of grids (per tensor object / storage / version) and every
    # launch that follows reads the tiles: half the grid traffic per step.  Pays when a batch of grids is used for more launches than the
    # tiling pass costs (one read + one write of the grids: ~0.4 ms per GiB; ~3 us saved per launch at B = 4096) -- the TBPTT window of learning/train_planner.py
    # re-uses one batch for every iteration of a window.  Off by default: a single step() per batch of grids would lose.  Grids that are already tiled, shared
    # (expand()ed) grids and trajectories of more than 128 states are left alone.
    self.auto_tile = False
    self._tile_cache = None            # (weakref to the row-major tensor, data_ptr, version, shape, dtype) -> its TiledSdf
    self.last_info = None
    self._last = None
    self._solvers = {}                 # torch dtype -> _capi.Solver
    self._planar = {}                  # torch dtype -> the planar companion _capi.Solver of a dof 3 layer (_planar_solver)
    self._sdf_cache = None             # marshalled arguments of the last SDF tensor seen (see _sdf_args)
    self._err_protos = {}              # (B, dtype, device index) -> (B,1,1) prototype for torch.empty_like
    self._info_bufs = {}               # (B, device index, raw stream) -> the int32 flag buffer launches on that stream write
    q = gp_params['Q_c_inv']
    self._qc_rows = [[float(v) for v in row] for row in (q.tolist() if torch.is_tensor(q) else q)]
    # DGP_QC_SCALAR scales the configuration's Q_c_inv: q_k^2 I (diag_identity) is that only for Q_c_inv = I
    self._scalar_qc = all(self._qc_rows[i][j] == (1.0 if i == j else 0.0) for i in range(len(self._qc_rows)) for j in range(len(self._qc_rows)))
    self._pc = _capi.get_pycall()      # fails loudly if the library / trampoline have not been built
    self._solver(torch.float64)        # validates the configuration now

  # -- C-ABI plumbing -------------------------------------------------------------------------------
  def _solver(self, dtype):
    s = self._solvers.get(dtype)
    if s is None:
      code = _io_code(dtype)
      gp, ob = self.gp_params, self.obs_params
      cfg = _capi.make_config(
          num_states=self.num_traj_states, dof=self.dof, io_dtype=code, total_time_sec=_f(self.total_time_sec),
          x_lims=[_f(v) for v in self.env_params['x_lims']], y_lims=[_f(v) for v in self.env_params['y_lims']],
          K_s=_f(gp['K_s']), K_g=_f(gp['K_g']), reg=_f(self.optim_params['reg']), sphere_radius=_f(self.robot_model.get_sphere_radii()),
          Q_c_inv=self._qc_rows, cost_sigma=_f(ob['cost_sigma']), epsilon_dist=_f(ob['epsilon_dist']),
          non_holonomic=self.non_holonomic, use_vel_limits=self.use_vel_limits,
          K_d=_f(gp['K_d']) if self.non_holonomic else 0.0, K_v=_f(gp['K_v']) if self.use_vel_limits else 0.0,
          v_x=_f(gp['v_x']) if self.use_vel_limits else 0.0, v_y=_f(gp['v_y']) if self.use_vel_limits else 0.0, nlinks=self.nlinks)
      s = _capi.Solver(cfg)
      assert s.M == self.M
      self._solvers[dtype] = s
    return s

  def _planar_solver(self, dtype):
    """The handle the planar side kernels (dgp_sample_problems, dgp_init_paths, dgp_shortcut_paths: dof 2 only) run on.  A dof 2 layer: its own.  The x-y-heading
    robot (dof 3): a planar COMPANION handle, built once per dtype and kept -- the same num_states, I/O type, total_time_sec, limits, sphere_radius, epsilon_dist,
    cost_sigma, K_s, K_g and reg, the top-left 2 x 2 of Q_c_inv, no flags; what those kernels return goes through lift_headings."""
    if self.dof == 2: return self._solvers.get(dtype) or self._solver(dtype)
    s = self._planar.get(dtype)
    if s is None:
      gp, ob = self.gp_params, self.obs_params
      cfg = _capi.make_config(
          num_states=self.num_traj_states, dof=2, io_dtype=_io_code(dtype), total_time_sec=_f(self.total_time_sec),
          x_lims=[_f(v) for v in self.env_params['x_lims']], y_lims=[_f(v) for v in self.env_params['y_lims']],
          K_s=_f(gp['K_s']), K_g=_f(gp['K_g']), reg=_f(self.optim_params['reg']), sphere_radius=_f(self.robot_model.get_sphere_radii()),
          Q_c_inv=[row[:2] for row in self._qc_rows[:2]], cost_sigma=_f(ob['cost_sigma']), epsilon_dist=_f(ob['epsilon_dist']), nlinks=self.nlinks)
      s = self._planar[dtype] = _capi.Solver(cfg)
    return s

  def _err_proto(self, B, dtype, dev, like):
    """A (B,1,1) tensor whose only purpose is to be the argument of torch.empty_like (the cheapest way to allocate err / err_ext)."""
    if len(self._err_protos) > 64: self._err_protos.clear()
    t = self._err_protos[(B, dtype, dev)] = torch.empty((B, 1, 1), dtype=dtype, device=like.device)
    return t

  def _info_buffer(self, B, dev, stream, like):
    """The (B) int32 SPD flags a launch writes (`last_info`).  One buffer per (batch, device, stream), reused by the next forward() on
    that stream (stream order makes that safe; clone() `last_info` to keep it across calls)."""
    k = (B, dev, stream)
    t = self._info_bufs.get(k)
    if t is None:
      if len(self._info_bufs) > 64: self._info_bufs.clear()
      t = self._info_bufs[k] = torch.empty(B, dtype=torch.int32, device=like.device)
    return t

  def _sdf_args(self, sdfb, dtype, B, dev):
    """sdfb (B,1,H,W) (only channel 0 is read, obstacle_cost.py:35) -> the seven DgpSdf fields (address, H, W, batch stride in elements, layout, 0, None) + a keep-alive tensor; an
    expand()ed / single grid is passed as shared (stride 0).  None: no grid (dgp_eval_errors without obstacle outputs only).
    A GN loop passes the same grid tensor every iteration, and slicing + checking it costs 5 us -- half a kernel -- so the result for
    the LAST tensor seen is cached, but ONLY in the zero-copy case: the kernel then reads sdfb's own storage, whatever was written to
    it and however (in place, through .data, through an aliasing numpy / DLPack buffer), so the entry cannot go stale; it is keyed on
    the tensor object, its storage address, shape, strides, dtype and the batch.  A grid that needs a converted copy (other dtype than
    thb, non-contiguous) is converted on EVERY call, on the current stream, like any other torch op."""
    if sdfb is None:
      return _NO_SDF
    c = self._sdf_cache
    if (c is not None and c[0]() is sdfb and c[1] == sdfb.data_ptr() and c[2] == sdfb.shape and c[3] == sdfb.stride() and c[4] is sdfb.dtype
        and c[5] == B and c[6] == dev and c[7] is dtype):
      return c[8]
    _require_cuda(sdfb, 'sdfb')
    if sdfb.get_device() != dev: _same_device(dev, sdfb=sdfb)
    if sdfb.dim() == 6 and sdfb.shape[-2:] == (4, 4): return self._tiled_sdf_args(sdfb, dtype, B, dev)      # utils.sdf_utils.tile_sdf / sdf_2d_batch(layout='tiled4')
    if sdfb.dim() != 4: raise ValueError('sdfb must be (B,1,H,W) (or the (B,1,H/4,W/4,4,4) tiles of utils.sdf_utils.tile_sdf)')
    H, W = sdfb.shape[-2], sdfb.shape[-1]
    shared = sdfb.stride(0) == 0 or sdfb.shape[0] == 1
    if not shared and sdfb.shape[0] != B:       # a per-sample grid tensor with fewer grids than trajectories would be read out of bounds
      raise ValueError('sdfb has %d grids for a batch of %d trajectories (expected %d, or 1 / an expand()ed view for a shared grid)'
                       % (sdfb.shape[0], B, B))
    t = sdfb[0:1, 0:1] if shared else sdfb[:, 0:1]
    t = t.detach()
    if t.dtype != dtype or not t.is_contiguous():
      t = t.to(dtype).contiguous()              # an owned copy: never cached (it would not see later writes to sdfb)
      return (t.data_ptr(), int(H), int(W), 0 if shared else int(t.stride(0)), _capi.DGP_SDF_ROWMAJOR, 0, None, t)
    res = (t.data_ptr(), int(H), int(W), 0 if shared else int(t.stride(0)), _capi.DGP_SDF_ROWMAJOR, 0, None, None)      # a view into sdfb: lives as long as sdfb does
    me = weakref.ref(self)

    def _drop(_, me=me):                        # the tensor died: its address may be reused by another tensor object
      s = me()
      if s is not None: s.__dict__['_sdf_cache'] = None
    try:
      self.__dict__['_sdf_cache'] = (weakref.ref(sdfb, _drop), sdfb.data_ptr(), sdfb.shape, sdfb.stride(), sdfb.dtype, B, dev, dtype, res)
    except TypeError:
      self.__dict__['_sdf_cache'] = None
    return res[:7] + (t,)                       # (the caller's copy of the result keeps the view alive for the duration of the call)

  def _auto_tiled(self, sdfb, B):
    """auto_tile: sdfb as the launches should see it -- its cached 4 x 4-tiled copy when it is a per-sample row-major batch of grids, sdfb itself otherwise.  With
    requires_grad the tiles enter the graph through _AutoTile, so gradients come back in sdfb's own (row-major) shape."""
    if (sdfb is None or sdfb.dim() != 4 or sdfb.shape[0] != B or B == 1 or sdfb.stride(0) == 0 or sdfb.shape[1] != 1 or self.num_traj_states > 128
        or sdfb.dtype not in (torch.float32, torch.float64)):
      return sdfb
    c = self._tile_cache
    # (under HIP-graph capture the tiling pass is recorded with everything else and re-run by every replay -- a cached copy would go stale when the caller writes new
    #  grids into the captured tensor: give a graphed iteration pre-tiled grids instead, PlanningDataset(sdf_layout='tiled4') / tile_sdf)
    capturing = sdfb.is_cuda and torch.cuda.is_current_stream_capturing()
    if capturing or not (c is not None and c[0]() is sdfb and c[1] == sdfb.data_ptr() and c[2] == sdfb._version and c[3] == sdfb.shape and c[4] is sdfb.dtype):
      from ..utils.sdf_utils import tile_sdf
      with torch.no_grad():
        tiles = tile_sdf(sdfb.detach())
      if capturing:
        if sdfb.requires_grad and torch.is_grad_enabled():
          out = _AutoTile.apply(sdfb, tiles)
          out.__dict__.setdefault('_dgp_hw', tiles.__dict__['_dgp_hw'])
          return out
        return tiles
      me = weakref.ref(self)

      def _drop(_, me=me):
        s_ = me()
        if s_ is not None: s_.__dict__['_tile_cache'] = None
      try: c = (weakref.ref(sdfb, _drop), sdfb.data_ptr(), sdfb._version, sdfb.shape, sdfb.dtype, tiles)
      except TypeError: return sdfb
      self.__dict__['_tile_cache'] = c
    tiles = c[5]
    if sdfb.requires_grad and torch.is_grad_enabled():
      out = _AutoTile.apply(sdfb, tiles)
      if '_dgp_hw' not in out.__dict__: out.__dict__['_dgp_hw'] = tiles.__dict__['_dgp_hw']
      return out
    return tiles

  def _tiled_sdf_args(self, sdfb, dtype, B, dev):
    """A grid stored as 4 x 4 tiles, (B | 1, 1, Ht, Wt, 4, 4) contiguous per grid (utils.sdf_utils.tile_sdf): -> the DgpSdf fields with layout DGP_SDF_TILED4.  The
    logical size (H, W) -- it sets the resolution and the clamping of the lookup, and the tile counts do not determine it (130 and 132 both give 33 tiles) -- comes
    from the tensor (a utils.sdf_utils.TiledSdf carries it through .to() / .detach() / indexing / collation) or, for a plain tensor that lost it, from
    `self.sdf_hw`; without either the call is refused rather than guessed.  Not cached: the checks are cheap next to a kernel on per-sample grids."""
    hw = sdfb.__dict__.get('_dgp_hw') or self.sdf_hw
    with torch._C.DisableTorchFunctionSubclass():      # (a TiledSdf: no __torch_function__ round trip per attribute below)
      if sdfb.shape[1] != 1: raise ValueError('tiled sdfb must be (B,1,Ht,Wt,4,4)')
      Ht, Wt = int(sdfb.shape[2]), int(sdfb.shape[3])
      if hw is None:
        raise ValueError('tiled sdfb (B,1,%d,%d,4,4) carries no logical grid size: it is not a utils.sdf_utils.TiledSdf (tile_sdf / sdf_2d_batch(layout="tiled4") return one; '
                         'as_tiled(t, (H, W)) re-declares tiles that went through foreign code) and plan_layer.sdf_hw is not set.  The size cannot be guessed: '
                         '%d x %d tiles hold any grid from %d x %d to %d x %d, and H, W set the resolution and the clamping of the lookup' %
                         (Ht, Wt, Ht, Wt, 4 * Ht - 3, 4 * Wt - 3, 4 * Ht, 4 * Wt))
      H, W = int(hw[0]), int(hw[1])
      if (H + 3) // 4 != Ht or (W + 3) // 4 != Wt: raise ValueError('tiled sdfb of %d x %d tiles does not hold a %d x %d grid' % (Ht, Wt, H, W))
      shared = sdfb.stride(0) == 0 or sdfb.shape[0] == 1
      if not shared and sdfb.shape[0] != B:
        raise ValueError('sdfb has %d grids for a batch of %d trajectories (expected %d, or 1 / an expand()ed view for a shared grid)' % (sdfb.shape[0], B, B))
      t = (sdfb[0:1] if shared else sdfb).detach()
      if t.dtype != dtype or not t.is_contiguous(): t = t.to(dtype).contiguous()
      return (t.data_ptr(), H, W, 0 if shared else Ht * Wt * 16, _capi.DGP_SDF_TILED4, 0, None, t)

  @staticmethod
  def static_flags(qc, ow, eps):
    """(qc, ow, eps) -> which of them stand for the handle's static constants: None, or a tensor that
    DiffGPMP2Planner tagged as the expand()ed view of its own static covariance."""
    return (qc is None or '_dgp_static' in qc.__dict__, ow is None or '_dgp_static' in ow.__dict__, eps is None or '_dgp_static' in eps.__dict__)

  def _cov_args(self, qc, ow, eps, dtype, B, dev, static=(False, False, False), scalar_ok=False):
    """Covariance tensors -> the four DgpCovs fields (qc_mode, the qc_inv / obs_w / eps addresses) + a keep-alive list.  A static entry selects the constants of the
    handle (no per-state tensor is streamed)."""
    if static == _ALL_STATIC:
      return _NO_COVS_KEEP
    n, dof, d = self.num_traj_states, self.dof, self.state_dim
    keep = []

    def prep(t, count, name):
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
      if t.shape[0] != B: raise ValueError('%s has batch %d, expected %d' % (name, t.shape[0], B))
      if t.numel() != B * count: raise ValueError('%s has %d elements, expected %d' % (name, t.numel(), B * count))
      if t.dtype is not dtype: t = t.to(dtype)
      t = t.contiguous()
      keep.append(t)
      return t.data_ptr()

    mode, qc_p, ow_p, ep_p = _capi.DGP_QC_STATIC, None, None, None
    if qc is not None and not static[0]:
      # scalar_ok (step() / step_with_errors(), forward and backward launches): a tensor the planner tagged as q_k^2 I (dynamics_mode 'diag_identity') goes down as its
      # n - 1 scalars; the gradient the backward kernel writes is that of the (B,n-1,dof,dof) blocks all the same
      tag = qc.__dict__.get('_dgp_scalar') if (scalar_ok and self._scalar_qc and not self._q_full and n <= 256) else None
      sc = tag[0] if (tag is not None and tag[1] == qc._version) else None
      if sc is not None and sc.shape == (B, n - 1):
        mode = _capi.DGP_QC_SCALAR
        qc_p = prep(sc, n - 1, 'qc_inv_trajb (one scalar per GP factor)')
      else:
        mode = _capi.DGP_QC_QFULL if self._q_full else _capi.DGP_QC_PERSTATE
        qc_p = prep(qc, (n - 1) * (d * d if self._q_full else dof * dof), 'qc_inv_trajb')
    if ow is not None and not static[1]: ow_p = prep(ow, n * self.nlinks, 'obscov_inv_trajb')
    if eps is not None and not static[2]: ep_p = prep(eps, n * self.nlinks, 'eps_trajb')
    return (mode, qc_p, ow_p, ep_p, keep)

  def _check_inputs(self, thb, startb, goalb):
    if not (thb.is_cuda and startb.is_cuda and goalb.is_cuda):
      _require_cuda(thb, 'thb'); _require_cuda(startb, 'startb'); _require_cuda(goalb, 'goalb')
    shp = thb.shape
    if len(shp) != 3 or shp[1] != self.num_traj_states or shp[2] != self.state_dim:
      raise ValueError('thb must be (B,%d,%d), got %s' % (self.num_traj_states, self.state_dim, tuple(thb.shape)))
    nd = shp[0] * self.state_dim
    if startb.numel() != nd or goalb.numel() != nd:
      raise ValueError('startb/goalb must be (B,1,%d)' % self.state_dim)
    dt = thb.dtype
    if startb.dtype is not dt or goalb.dtype is not dt:
      raise TypeError('thb, startb, goalb must share one dtype')

  def _remember(self, startb, goalb, static, qc, ow, eps):
    """Like the reference (plan_layer.py:88-94) remember means / covariances for the error_* helpers below.  start / goal / eps are kept WITH their graphs,
    as set_mean / set_eps do: error_ext_batch and the unweighted errors are differentiable w.r.t. them; qc_inv / obscov_inv only feed error_batch, which runs
    under no_grad, :275."""
    if static == _ALL_STATIC:
      self.__dict__['_last'] = (startb, goalb, None, None, None)
    else:
      self.__dict__['_last'] = (startb, goalb, None if (qc is None or static[0]) else qc.detach(), None if (ow is None or static[1]) else ow.detach(),
                                None if (eps is None or static[2]) else eps)

  @staticmethod
  def _diff_slots(ts):
    """ts = every input of a node, the grid at ts[3] -> (ts as the node should see them -- a grid that requires grad through _expand_base --, slots: the
    indices of those that require grad; empty: no autograd node)."""
    sdfb = ts[3]
    if sdfb is not None and sdfb.requires_grad: ts = ts[:3] + (_expand_base(sdfb),) + ts[4:]
    return ts, tuple([i for i, t in enumerate(ts) if t is not None and t.requires_grad])

  # -- the reference's public surface -----------------------------------------------------------------
  def forward(self, thb, startb, goalb, imb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb):
    """plan_layer.py:87-99.  -> (dthetab (B,n,d), err (B,1,1) [no grad], err_ext (B,1,1) [grad])."""
    self._check_inputs(thb, startb, goalb)
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, thb.shape[0])
    static = self.static_flags(qc_inv_trajb, obscov_inv_trajb, eps_trajb)
    self._remember(startb, goalb, static, qc_inv_trajb, obscov_inv_trajb, eps_trajb)
    if torch.is_grad_enabled():
      ts, slots = self._diff_slots((thb, startb, goalb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb))
      if slots:
        box = []
        dth, eex = _GNStep.apply(self, static, slots, ts, box, *[ts[i] for i in slots])
        return dth, box[0], eex
    # planning / validation loops: no autograd node, one launch
    return _GNStep.launch(self, False, static, thb, startb, goalb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb)[:3]

  def forward_with_errors(self, thb, startb, goalb, imb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb):
    """forward() and, in the same call, what the reference's training loop evaluates right behind it (learning/train_planner.py:313,327):
    the unweighted errors of unweighted_errors_batch at thb + dthetab.  -> (dthetab, err, err_ext, err_sg (B,1), err_gp (B,1,1), err_obs (B,1,1));
    everything but err carries the graph (ONE autograd node, ONE backward call).  Equivalent to
        dth, err, eex = layer(thb, ...); sg, gp, ob = layer.unweighted_errors(thb + dth, sdfb)"""
    self._check_inputs(thb, startb, goalb)
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, thb.shape[0])
    B = thb.shape[0]
    if self.num_traj_states > 256:      # the fused entry points stop at 256 states: the two calls this method stands for (the loop kernels of gn_long.h)
      dth, err, eex = self.forward(thb, startb, goalb, imb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb)
      sg, gp, ob = self.unweighted_errors(thb + dth, sdfb)
      return dth, err, eex, sg, gp, ob
    static = self.static_flags(qc_inv_trajb, obscov_inv_trajb, eps_trajb)
    self._remember(startb, goalb, static, qc_inv_trajb, obscov_inv_trajb, eps_trajb)
    if torch.is_grad_enabled():
      ts, slots = self._diff_slots((thb, startb, goalb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb))
      if slots:
        box = []
        dth, eex, usg, ugp, uobs = _GNStepErrors.apply(self, static, slots, ts, box, *[ts[i] for i in slots])
        return dth, box[0], eex, usg.reshape(B, 1), ugp, uobs
    dth, err, eex, usg, ugp, uobs = _GNStep.launch(self, True, static, thb, startb, goalb, sdfb, qc_inv_trajb, obscov_inv_trajb, eps_trajb)[:6]
    return dth, err, eex, usg.reshape(B, 1), ugp, uobs

  def raw_covs(self, out, mode, learn_eps):
    """The learn module's output `out` as a covariance input the kernels square themselves (_RawCovs), or None when this call cannot take that path: single-link
    robot, dynamics_mode 'diag_identity' (with Q_c_inv = I in the configuration: q_k^2 I is then a scalar multiple of it) or 'fix_dynamics', out (B, 1, W) contiguous
    with W at least what the mode consumes, at most 256 states."""
    n = self.num_traj_states
    if self.nlinks != 1 or n > 256 or self._q_full or out.dim() != 3 or out.shape[1] != 1 or not out.is_contiguous(): return None
    if mode == 'diag_identity':
      if not self._scalar_qc: return None
      n_gp = n - 1
    elif mode == 'fix_dynamics': n_gp = 0
    else: return None
    raw = _RawCovs(out, n_gp, n, bool(learn_eps), self.dof)
    if learn_eps and raw.used != out.shape[2]: return None      # (the reference's reshape of the epsilon block would raise: keep its behaviour)
    if raw.used > out.shape[2]: return None
    return raw

  def forward_raw(self, thb, startb, goalb, imb, sdfb, raw, with_errors=False):
    """forward() / forward_with_errors() with the covariances given as the learn module's output vector (`raw` = self.raw_covs(out, mode, learn_eps)).
    -> (dthetab, err, err_ext[, err_sg (B,1), err_gp, err_obs], qc_inv_trajb or None, obscov_inv_trajb, eps_trajb or None): the last three are what
    get_covariances would have built (same values), carrying the graph to `out` like everything else."""
    self._check_inputs(thb, startb, goalb)
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, thb.shape[0])
    out = raw.out
    if out.dtype is not thb.dtype or out.get_device() != thb.get_device() or out.shape[0] != thb.shape[0]:
      raise ValueError('the learn module output must share dtype, device and batch with thb')
    B = thb.shape[0]
    if torch.is_grad_enabled():
      ts, slots = self._diff_slots((thb, startb, goalb, sdfb, out))
      if slots:
        box = []
        res = _GNStepRaw.apply(self, raw, with_errors, slots, ts, box, *[ts[i] for i in slots])
        err = box[0][0]
        k = 5 if with_errors else 2
        sq = list(res[k:])
        qc = sq.pop(0) if raw.n_gp else None
        ow = sq.pop(0)
        eps = sq.pop(0) if raw.learn_eps else None
        self.__dict__['_last'] = (startb, goalb, None if qc is None else qc.detach(), ow.detach(), eps)
        if with_errors: return res[0], err, res[1], res[2].reshape(B, 1), res[3], res[4], qc, ow, eps
        return res[0], err, res[1], qc, ow, eps
    raw.square(self._pc, thb.get_device())
    qc, ow, eps = raw.qc, raw.ow, raw.eps
    self.__dict__['_last'] = (startb, goalb, qc, ow, eps)
    dth, err, eex, usg, ugp, uobs = _GNStep.launch(self, with_errors, raw, thb, startb, goalb, sdfb, out, None, None)[:6]
    if with_errors: return dth, err, eex, usg.reshape(B, 1), ugp, uobs, qc, ow, eps
    return dth, err, eex, qc, ow, eps

  def _eval_launch(self, thb, sdfb, startb, goalb, qc, ow, eps):
    """One dgp_eval_errors launch -> ([err, err_ext, start_goal_error, gp_error, obs_error] (None where a grid is needed and sdfb is
    None), the contiguous inputs, the marshalled SDF / covariance arguments)."""
    B = thb.shape[0]
    dtype = thb.dtype
    solver = self._solvers.get(dtype) or self._solver(dtype)
    dev = thb.get_device()
    if dev < 0: _require_cuda(thb, 'thb')
    if startb.get_device() != dev or goalb.get_device() != dev: _same_device(dev, startb=startb, goalb=goalb)
    sd = self._sdf_args(sdfb, dtype, B, dev)
    cv = self._cov_args(qc, ow, eps, dtype, B, dev, self.static_flags(qc, ow, eps))
    grid = sdfb is not None
    thc, stc, goc = thb.contiguous(), startb.contiguous(), goalb.contiguous()
    proto = self._err_protos.get((B, dtype, dev))
    if proto is None: proto = self._err_proto(B, dtype, dev, thc)
    outs = [torch.empty_like(proto) if w else None for w in (grid, grid, True, True, grid)]
    _launch(dev, self._pc.eval_errors, solver.h, B, thc.data_ptr(), stc.data_ptr(), goc.data_ptr(), *sd[:7], *cv[:4], _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(outs[4]), _raw_stream(dev))
    return outs, thc, stc, goc, sd, cv

  def _eval(self, thb, sdfb, startb, goalb, qc, ow, eps):
    """-> [err, err_ext, start_goal_error, gp_error, obs_error]; without a grid (sdfb None) the three that read it are None."""
    return self._eval_launch(thb, sdfb, startb, goalb, qc, ow, eps)[0]

  def errors(self, thb, startb, goalb, sdfb, qc_inv_trajb=None, obscov_inv_trajb=None, eps_trajb=None):
    """(err, err_ext, start_goal_error, gp_error, obs_error), each (B,1,1), in one launch (dgp_eval_errors).  Unlike the
    reference (which reads the means/covariances left behind by the last forward()) everything is an argument."""
    self._check_inputs(thb, startb, goalb)
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, thb.shape[0])
    return tuple(self._eval(thb, sdfb, startb, goalb, qc_inv_trajb, obscov_inv_trajb, eps_trajb))

  def _last_or_raise(self):
    if getattr(self, '_last', None) is None:
      raise RuntimeError('call forward() first: like the reference, the error_* helpers use the start/goal means and the '
                         'covariances set by the last forward() (plan_layer.py:88-94)')
    return self._last

  def error_batch(self, thb, sdfb):
    """plan_layer.py:273-308: normalised factor-graph error at thb, no grad, with the covariances of the last forward()."""
    st, go, qc, ow, eps = self._last_or_raise()
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, thb.shape[0])
    with torch.no_grad():
      return self._eval(thb, sdfb, st, go, qc, ow, eps)[0]

  def _eval_diff(self, thb, sdfb, st, go, eps):
    """(err_ext, start_goal_error, gp_error, obs_error) at thb, each (B,1,1) (None where a grid is needed and sdfb is None), carrying
    the autograd graph the reference's plain torch ops would carry: w.r.t. thb, sdfb, the start / goal means and the current eps."""
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, thb.shape[0])
    if torch.is_grad_enabled():
      ts, slots = self._diff_slots((thb, st, go, sdfb, eps))
      if slots:
        return _EvalErrors.apply(self, slots, ts, *[ts[i] for i in slots])
    o = self._eval(thb, sdfb, st, go, None, None, eps)
    return o[1], o[2], o[3], o[4]

  def error_ext_batch(self, thb, sdfb):
    """plan_layer.py:310-345: same with the FIXED GP / obstacle weights and the current eps.  Differentiable w.r.t. thb, sdfb, the
    start / goal means and the eps tensor of the last forward()."""
    st, go, qc, ow, eps = self._last_or_raise()
    return self._eval_diff(thb, sdfb, st, go, eps)[0]

  def start_goal_error(self, thb):
    """plan_layer.py:384-388 (unweighted; (B,1): the reference's mean(dim=1) drops one of the two singleton dimensions)."""
    st, go, qc, ow, eps = self._last_or_raise()
    return self._eval_diff(thb, None, st, go, None)[1].reshape(thb.shape[0], 1)

  def gp_error(self, thb):
    """plan_layer.py:374-377 (unweighted, mean over the GP factors)."""
    st, go, qc, ow, eps = self._last_or_raise()
    return self._eval_diff(thb, None, st, go, None)[2]

  def obs_error(self, thb, sdfb):
    """plan_layer.py:379-382 (unweighted, mean over states; uses the eps of the last forward())."""
    st, go, qc, ow, eps = self._last_or_raise()
    return self._eval_diff(thb, sdfb, st, go, eps)[3]

  def unweighted_errors(self, thb, sdfb):
    """(start_goal_error (B,1), gp_error (B,1,1), obs_error (B,1,1)) in one launch (and one backward launch)."""
    st, go, qc, ow, eps = self._last_or_raise()
    o = self._eval_diff(thb, sdfb, st, go, eps)
    return o[1].reshape(thb.shape[0], 1), o[2], o[3]

  def trajectory_metrics(self, thb, sdfb, th_optb=None, eps=0.0, return_obs_error=False):
    """The validation metrics of every trajectory of the batch in ONE launch (dgp_traj_metrics): what learning/test_planner.py:299-334 computes per trajectory with
    gpfactor.get_error, obsfactor.get_error, smoothness_metrics, collision_metrics, the velocity-limit loop and three MSELoss calls.  thb (B,n,d), sdfb as for
    forward() (row-major, TiledSdf, expand()ed shared grids), th_optb (B,n,d) the expert trajectories or None, eps the epsilon of the METRICS obstacle factor (the
    reference builds it with 0.0, not obs_params['epsilon_dist']).  No autograd: inputs are detached.  -> TrajectoryMetrics."""
    if thb.dim() != 3 or thb.shape[1] != self.num_traj_states or thb.shape[2] != self.state_dim:
      raise ValueError('thb must be (B,%d,%d), got %s' % (self.num_traj_states, self.state_dim, tuple(thb.shape)))
    if sdfb is None: raise ValueError('trajectory_metrics needs the signed-distance grids (sdfb)')
    B, dtype = thb.shape[0], thb.dtype
    solver = self._solvers.get(dtype) or self._solver(dtype)
    dev = thb.get_device()
    if dev < 0: _require_cuda(thb, 'thb')
    if self.auto_tile: sdfb = self._auto_tiled(sdfb, B)
    sd = self._sdf_args(sdfb, dtype, B, dev)
    thc = thb.detach().contiguous()
    opt = None
    if th_optb is not None:
      if th_optb.shape != thb.shape: raise ValueError('th_optb must have the shape of thb %s, got %s' % (tuple(thb.shape), tuple(th_optb.shape)))
      if th_optb.dtype != dtype: raise TypeError('th_optb must have the dtype of thb (%s), got %s' % (dtype, th_optb.dtype))
      if th_optb.get_device() != dev: _same_device(dev, th_optb=th_optb)
      opt = th_optb.detach().contiguous()
    raw = torch.empty((B, _capi.DGP_METRIC_COUNT), dtype=torch.float64, device=thc.device)
    oerr = torch.empty((B, self.num_traj_states), dtype=dtype, device=thc.device) if return_obs_error else None
    _launch(dev, self._pc.traj_metrics, solver.h, B, thc.data_ptr(), *sd[:7], float(eps), _ptr(opt), raw.data_ptr(), _ptr(oerr), _raw_stream(dev))
    return TrajectoryMetrics(raw, oerr)

  def interpolate(self, thb, num_inter, sdfb=None, eps=0.0, return_cost=False):
    """The GP-interpolated dense trajectory of every trajectory of the batch -- num_inter states inside every interval, N_d = (n - 1)(num_inter + 1) + 1 in all --
    and, with sdfb, the collision check of every dense state, in ONE launch (dgp_gp_interpolate; include/dgpmp2_hip.h states the rule, utils.planner_utils.
    gp_interpolate_traj is its torch mirror).  The reference names the capability (gpmp2_planner.py:29-41: 'total_check_step', 'use_gp_inter') and never builds it.
    thb (B,n,d); sdfb as for trajectory_metrics (row-major, TiledSdf, expand()ed shared grids) or None: interpolation only; eps the epsilon of the check (a dense
    state collides where dist <= eps + sphere_radius).  No autograd: inputs are detached.  -> DenseTrajectory."""
    if thb.dim() != 3 or thb.shape[1] != self.num_traj_states or thb.shape[2] != self.state_dim:
      raise ValueError('thb must be (B,%d,%d), got %s' % (self.num_traj_states, self.state_dim, tuple(thb.shape)))
    K = int(num_inter)
    if K != num_inter or K < 0 or K > _capi.DGP_MAX_NUM_INTER: raise ValueError('num_inter must be an integer in 0..%d, got %r' % (_capi.DGP_MAX_NUM_INTER, num_inter))
    if return_cost and sdfb is None: raise ValueError('interpolate(return_cost=True) needs the signed-distance grids (sdfb)')
    B, dtype = thb.shape[0], thb.dtype
    solver = self._solvers.get(dtype) or self._solver(dtype)
    dev = thb.get_device()
    if dev < 0: _require_cuda(thb, 'thb')
    nd = (self.num_traj_states - 1) * (K + 1) + 1
    if sdfb is not None and nd < 3: raise ValueError('the collision summary needs at least 3 dense states, got %d' % nd)
    if sdfb is not None and self.auto_tile: sdfb = self._auto_tiled(sdfb, B)
    sd = self._sdf_args(sdfb, dtype, B, dev)
    thc = thb.detach().contiguous()
    dense = torch.empty((B, nd, self.state_dim), dtype=dtype, device=thc.device)
    raw = torch.empty((B, _capi.DGP_DENSE_COUNT), dtype=torch.float64, device=thc.device) if sdfb is not None else None
    cost = torch.empty((B, nd), dtype=dtype, device=thc.device) if return_cost else None
    _launch(dev, self._pc.gp_interpolate, solver.h, B, thc.data_ptr(), K, *sd[:7], float(eps), dense.data_ptr(), _ptr(cost), _ptr(raw), _raw_stream(dev))
    from ..utils.planner_utils import gp_interpolate_times
    times = gp_interpolate_times(_f(self.total_time_sec), self.total_time_step, K, dtype=torch.float64, device=thc.device)
    return DenseTrajectory(dense, times, raw, cost)

  def step_loss(self, dthetab, th_currb, th_optb, errors, weights=None):
    """The loss of one training iteration on the device (dgp_step_loss; include/dgpmp2_hip.h states it, utils.learn_utils.one_step_loss_torch is its torch mirror):
    the reference's one_step_loss(dthetab, th_optb - th_currb, ...) (learning/train_planner.py:75-120, :328) with the subtraction folded in -- the miss is
    dthetab - (th_optb - th_currb) -- and one autograd node whose backward is one launch.  dthetab, th_currb, th_optb (B,n,d); errors = (err_sg, err_gp, err_obs) as
    step_with_errors / unweighted_errors_batch return them (an entry may be None: a zero term); weights: learn_params['optim'] by default (the keys vel_loss_lambda,
    ext_obs_lambda, ext_loss_weight).  Positions are columns [0, dof), velocities [dof, d): for dof 2 the reference's hard-coded columns 0,1 / 2,3, for dof 3 NOT
    what the reference's text would pick (theta and v_x as "velocity", v_y and omega ignored; its training loop only runs dof 2).  -> LossTerms(total, pos, vel, cov, gp,
    sg, obs, ext), 0-d float64 tensors (`total` differentiable w.r.t. all six inputs), with `.per_sample` (B,5) and `.raw` (8,).  Usable inside graphed_iteration /
    torch.cuda.graph."""
    if weights is None:
      if self.learn_params is None or 'optim' not in self.learn_params: raise ValueError("step_loss needs `weights` (or learn_params['optim'])")
      weights = self.learn_params['optim']
    if dthetab.dim() != 3 or dthetab.shape[1] != self.num_traj_states or dthetab.shape[2] != self.state_dim:
      raise ValueError('dthetab must be (B,%d,%d), got %s' % (self.num_traj_states, self.state_dim, tuple(dthetab.shape)))
    return device_step_loss(self._pc, self.dof, dthetab, th_optb, th_currb, errors, weights)

  def check_solved(self, thb, sdfb, clearance=None):
    """Whether every state of a trajectory keeps clear of the obstacles, for the whole batch in ONE launch (dgp_sdf_lookup's summary; the test of the reference's
    check_solved, learning/train_initializer.py:81-88): -> (B,) bool device tensor, True where NO state has a signed distance d_obs <= clearance at its position.
    thb (B,n,d), read in place; sdfb as for forward() (row-major, TiledSdf, expand()ed shared grids); clearance: the sphere radius by default.  The resolution is
    taken from the padded width of sdfb, as the planner's own obstacle factor takes it (obstacle_cost.py:34) -- utils.learn_utils.check_solved takes the
    reference's explicit cell size instead.  Unlike trajectory_metrics' in_collision, the first and the last state count, and the threshold carries no epsilon.
    Does not depend on num_traj_states.  No autograd, no synchronisation; usable inside torch.cuda.graph."""
    from .sdf_lookup import device_sdf_lookup
    if thb.dim() != 3 or thb.shape[2] < 2: raise ValueError('thb must be (B,n,d), got %s' % (tuple(thb.shape),))
    if sdfb is None: raise ValueError('check_solved needs the signed-distance grids (sdfb)')
    hw = sdfb.__dict__.get('_dgp_hw') if sdfb.dim() == 6 else None
    W = int(hw[1]) if hw is not None else int(sdfb.shape[-1])
    if sdfb.dim() == 6 and hw is None:
      if self.sdf_hw is None: raise ValueError('tiled sdfb carries no logical grid size (utils.sdf_utils.TiledSdf) and plan_layer.sdf_hw is not set')
      from ..utils.sdf_utils import as_tiled
      sdfb, W = as_tiled(sdfb, self.sdf_hw), int(self.sdf_hw[1])
    x_lims, y_lims = [_f(v) for v in self.env_params['x_lims']], [_f(v) for v in self.env_params['y_lims']]
    res = (x_lims[1] - x_lims[0]) / W
    r = _f(self.robot_model.get_sphere_radii()) if clearance is None else _f(clearance)
    if sdfb.dtype is not thb.dtype: sdfb = sdfb.to(thb.dtype)
    return device_sdf_lookup(sdfb, thb, res, x_lims, y_lims, r, want_d=False, want_J=False).solved

  def sample_problems(self, sdfb, num_problems, params, dtype=torch.float64, env_index=None, diagonal=None, seed=0, first_problem=0):
    """Feasible start / goal pairs and their straight-line initial trajectories in ONE launch (dgp_sample_problems; datasets.problem_generation.sample_problems is the
    documented front end and fills `params`, a _capi.DgpSampleParams).  sdfb as for forward() (row-major, TiledSdf, a shared grid); env_index (B) int32 device tensor:
    the grid of sdfb each problem is sampled in (None: grid b / the shared grid), diagonal (B) int32 device tensor or None.
    -> startb, goalb (B,1,4), th_initb (B,n,4) of `dtype`, draws (B,2) int32, info (B) int32, all on sdfb's device."""
    if sdfb is None: raise ValueError('sample_problems needs the signed-distance grids (sdfb)')
    _require_cuda(sdfb, 'sdfb')
    B, dev = int(num_problems), sdfb.get_device()
    solver = self._planar_solver(dtype)
    grids = int(sdfb.shape[0])
    shared = grids == 1 or sdfb.stride(0) == 0
    if env_index is None and not shared and grids != B:
      raise ValueError('sdfb has %d grids for %d problems: pass env_index (the grid of each problem)' % (grids, B))
    sd = self._sdf_args(sdfb, dtype, B if (shared or env_index is None) else grids, dev)
    keep = []

    def index_arg(t, name):
      if t is None: return None
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
      if t.dtype is not torch.int32 or t.dim() != 1 or t.shape[0] != B: raise ValueError('%s must be an int32 tensor of shape (%d,), got %s %s' % (name, B, t.dtype, tuple(t.shape)))
      t = t.contiguous()
      keep.append(t)
      return t.data_ptr()
    ei, dg = index_arg(env_index, 'env_index'), index_arg(diagonal, 'diagonal')
    device = sdfb.device
    startb = torch.empty((B, 1, 4), dtype=dtype, device=device)
    goalb = torch.empty((B, 1, 4), dtype=dtype, device=device)
    th_initb = torch.empty((B, self.num_traj_states, 4), dtype=dtype, device=device)
    draws = torch.empty((B, 2), dtype=torch.int32, device=device)
    info = torch.empty((B,), dtype=torch.int32, device=device)
    import ctypes
    api = _capi.get_api()
    arg = _capi.DgpSdf(*sd[:7])
    _launch(dev, api.sample_problems, solver.h, B, ctypes.byref(arg), ei, ctypes.byref(params), int(seed), int(first_problem), dg, startb.data_ptr(), goalb.data_ptr(),
            th_initb.data_ptr(), draws.data_ptr(), info.data_ptr(), _raw_stream(dev))
    return startb, goalb, th_initb, draws, info

  def init_paths(self, sdfb, startb, goalb, params, dtype=torch.float64, env_index=None, field=None):
    """Collision-free initial trajectories from startb to goalb in ONE launch (dgp_init_paths; datasets.problem_generation.init_paths is the documented front end, fills
    `params`, a _capi.DgpPathParams, and chunks a large batch).  sdfb: ROW-MAJOR grids as for forward() (per sample, a shared grid, or several addressed through
    env_index (B) int32); startb / goalb (B,1,4).  field: a (B,H,W) int32 device tensor to use as the distance-field workspace (the bits of the uint32 field), or None.
    -> th_initb (B,n,4) of `dtype`, field (B,H,W) int32, path_cells (B,path_cap) int32, num_cells (B) int32, length (B) float64, info (B) int32."""
    if sdfb is None: raise ValueError('init_paths needs the signed-distance grids (sdfb)')
    _require_cuda(sdfb, 'sdfb')
    if sdfb.dim() == 6: raise ValueError('init_paths reads row-major grids: untile a TiledSdf first (utils.sdf_utils.untile_sdf)')
    B, dev = int(startb.shape[0]), sdfb.get_device()
    for name, t in (('startb', startb), ('goalb', goalb)):
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
      if tuple(t.shape) != (B, 1, 4): raise ValueError('%s must be (B,1,4), got %s' % (name, tuple(t.shape)))
    solver = self._planar_solver(dtype)
    grids = int(sdfb.shape[0])
    shared = grids == 1 or sdfb.stride(0) == 0
    if env_index is None and not shared and grids != B:
      raise ValueError('sdfb has %d grids for %d problems: pass env_index (the grid of each problem)' % (grids, B))
    sd = self._sdf_args(sdfb, dtype, B if (shared or env_index is None) else grids, dev)
    ei = None
    if env_index is not None:
      _require_cuda(env_index, 'env_index')
      if env_index.get_device() != dev: _same_device(dev, env_index=env_index)
      if env_index.dtype is not torch.int32 or env_index.dim() != 1 or env_index.shape[0] != B:
        raise ValueError('env_index must be an int32 tensor of shape (%d,), got %s %s' % (B, env_index.dtype, tuple(env_index.shape)))
      ei = env_index.contiguous()
    H, W = int(sd[1]), int(sd[2])
    device = sdfb.device
    st, go = startb.detach().to(dtype).contiguous(), goalb.detach().to(dtype).contiguous()
    if field is None: field = torch.empty((B, H, W), dtype=torch.int32, device=device)
    elif tuple(field.shape) != (B, H, W) or field.dtype is not torch.int32 or not field.is_contiguous() or field.get_device() != dev:
      raise ValueError('field must be a contiguous (%d,%d,%d) int32 tensor on the device of sdfb' % (B, H, W))
    th_initb = torch.empty((B, self.num_traj_states, 4), dtype=dtype, device=device)
    cap = int(params.path_cap)
    path_cells = torch.empty((B, cap), dtype=torch.int32, device=device)
    num_cells = torch.empty((B,), dtype=torch.int32, device=device)
    info = torch.empty((B,), dtype=torch.int32, device=device)
    length = torch.empty((B,), dtype=torch.float64, device=device)
    import ctypes
    api = _capi.get_api()
    arg = _capi.DgpSdf(*sd[:7])
    _launch(dev, api.init_paths, solver.h, B, ctypes.byref(arg), _ptr(ei), ctypes.byref(params), st.data_ptr(), go.data_ptr(), th_initb.data_ptr(), field.data_ptr(),
            path_cells.data_ptr() if cap > 0 else None, num_cells.data_ptr(), length.data_ptr(), info.data_ptr(), _raw_stream(dev))
    return th_initb, field, path_cells, num_cells, length, info

  def shortcut_paths(self, sdfb, startb, goalb, thb, path_cells, num_cells, params, dtype=torch.float64, env_index=None):
    """Line-of-sight shortcutting of the grid paths of init_paths in ONE launch (dgp_shortcut_paths; datasets.problem_generation.shortcut_paths is the documented
    front end and fills `params`, a _capi.DgpShortcutParams).  sdfb, startb, goalb, env_index as for init_paths; thb (B,n,4) of `dtype`, contiguous, REWRITTEN in
    place for every simplified problem; path_cells (B,path_cap) and num_cells (B) int32 as init_paths returned them.
    -> vertex_index (B,vertex_cap) int32, num_vertices (B) int32, length (B) float64, info (B) int32."""
    if sdfb is None: raise ValueError('shortcut_paths needs the signed-distance grids (sdfb)')
    _require_cuda(sdfb, 'sdfb')
    if sdfb.dim() == 6: raise ValueError('shortcut_paths reads row-major grids: untile a TiledSdf first (utils.sdf_utils.untile_sdf)')
    B, dev = int(startb.shape[0]), sdfb.get_device()
    for name, t in (('startb', startb), ('goalb', goalb), ('thb', thb), ('path_cells', path_cells), ('num_cells', num_cells)):
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
    for name, t in (('startb', startb), ('goalb', goalb)):
      if tuple(t.shape) != (B, 1, 4): raise ValueError('%s must be (B,1,4), got %s' % (name, tuple(t.shape)))
    cap, vcap = int(params.path_cap), int(params.vertex_cap)
    if tuple(thb.shape) != (B, self.num_traj_states, 4) or thb.dtype is not dtype or not thb.is_contiguous():
      raise ValueError('thb must be a contiguous (%d,%d,4) tensor of %s, got %s %s' % (B, self.num_traj_states, dtype, tuple(thb.shape), thb.dtype))
    if tuple(path_cells.shape) != (B, cap) or path_cells.dtype is not torch.int32 or not path_cells.is_contiguous():
      raise ValueError('path_cells must be a contiguous int32 tensor of shape (%d,%d) (params.path_cap columns), got %s %s' % (B, cap, path_cells.dtype, tuple(path_cells.shape)))
    if tuple(num_cells.shape) != (B,) or num_cells.dtype is not torch.int32 or not num_cells.is_contiguous():
      raise ValueError('num_cells must be a contiguous int32 tensor of shape (%d,), got %s %s' % (B, num_cells.dtype, tuple(num_cells.shape)))
    solver = self._planar_solver(dtype)
    grids = int(sdfb.shape[0])
    shared = grids == 1 or sdfb.stride(0) == 0
    if env_index is None and not shared and grids != B:
      raise ValueError('sdfb has %d grids for %d problems: pass env_index (the grid of each problem)' % (grids, B))
    sd = self._sdf_args(sdfb, dtype, B if (shared or env_index is None) else grids, dev)
    ei = None
    if env_index is not None:
      _require_cuda(env_index, 'env_index')
      if env_index.get_device() != dev: _same_device(dev, env_index=env_index)
      if env_index.dtype is not torch.int32 or env_index.dim() != 1 or env_index.shape[0] != B:
        raise ValueError('env_index must be an int32 tensor of shape (%d,), got %s %s' % (B, env_index.dtype, tuple(env_index.shape)))
      ei = env_index.contiguous()
    device = sdfb.device
    st, go = startb.detach().to(dtype).contiguous(), goalb.detach().to(dtype).contiguous()
    vertex_index = torch.empty((B, vcap), dtype=torch.int32, device=device)
    num_vertices = torch.empty((B,), dtype=torch.int32, device=device)
    info = torch.empty((B,), dtype=torch.int32, device=device)
    length = torch.empty((B,), dtype=torch.float64, device=device)
    import ctypes
    api = _capi.get_api()
    arg = _capi.DgpSdf(*sd[:7])
    _launch(dev, api.shortcut_paths, solver.h, B, ctypes.byref(arg), _ptr(ei), ctypes.byref(params), st.data_ptr(), go.data_ptr(), path_cells.data_ptr(),
            num_cells.data_ptr(), thb.data_ptr(), vertex_index.data_ptr() if vcap > 0 else None, num_vertices.data_ptr(), length.data_ptr(), info.data_ptr(),
            _raw_stream(dev))
    return vertex_index, num_vertices, length, info

  def prior_samples(self, startb, goalb, num_samples, dtype=None, mean=None, scale=1.0, seed=0, first_problem=0, noise=None, return_noise=False):
    """num_samples trajectories per problem from the GP prior between startb and goalb in ONE launch (dgp_prior_samples; datasets.problem_generation.prior_samples is
    the documented front end).  startb / goalb (B,1,d); mean (B,n,d) or None: the prior mean; noise (B,S,n+1,d) float64 standard normals or None: generated on the
    device from (seed, first_problem + b, s).  -> th (B,S,n,d) of `dtype` (default: startb's), the (B,S,n+1,d) float64 normals used (None unless return_noise),
    info (B,S) int32: bit 0 a position outside the limits, bit 1 a non-finite value."""
    _require_cuda(startb, 'startb')
    B, S, d, n, dev = int(startb.shape[0]), int(num_samples), self.state_dim, self.num_traj_states, startb.get_device()
    if dtype is None: dtype = startb.dtype
    if S != num_samples or S < 1 or S > _capi.DGP_MAX_PRIOR_SAMPLES: raise ValueError('num_samples must be an integer in 1..2^24, got %r' % (num_samples,))
    if not (float(scale) >= 0.0) or float(scale) == float('inf'): raise ValueError('scale must be finite and >= 0, got %r' % (scale,))
    for name, t in (('startb', startb), ('goalb', goalb)):
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
      if tuple(t.shape) != (B, 1, d): raise ValueError('%s must be (%d,1,%d), got %s' % (name, B, d, tuple(t.shape)))
    solver = self._solvers.get(dtype) or self._solver(dtype)
    st, go = startb.detach().to(dtype).contiguous(), goalb.detach().to(dtype).contiguous()
    mn = None
    if mean is not None:
      _require_cuda(mean, 'mean')
      if mean.get_device() != dev: _same_device(dev, mean=mean)
      if tuple(mean.shape) != (B, n, d): raise ValueError('mean must be (%d,%d,%d), got %s' % (B, n, d, tuple(mean.shape)))
      mn = mean.detach().to(dtype).contiguous()
    nz = None
    if noise is not None:
      _require_cuda(noise, 'noise')
      if noise.get_device() != dev: _same_device(dev, noise=noise)
      if tuple(noise.shape) != (B, S, n + 1, d): raise ValueError('noise must be (%d,%d,%d,%d): n + 1 rows of d standard normals per sample, got %s' % (B, S, n + 1, d, tuple(noise.shape)))
      nz = noise.detach().to(torch.float64).contiguous()
    device = startb.device
    th = torch.empty((B, S, n, d), dtype=dtype, device=device)
    noise_out = torch.empty((B, S, n + 1, d), dtype=torch.float64, device=device) if return_noise else None
    info = torch.empty((B, S), dtype=torch.int32, device=device)
    _launch(dev, self._pc.prior_samples, solver.h, B, S, st.data_ptr(), go.data_ptr(), _ptr(mn), float(scale), int(seed), int(first_problem), _ptr(nz), th.data_ptr(),
            _ptr(noise_out), info.data_ptr(), _raw_stream(dev))
    return th, noise_out, info

  def heading_lift(self, th2b, params, dtype=None, start_heading=None, goal_heading=None, turns=None, return_turns=False):
    """Planar trajectories lifted to problems of the x-y-heading robot in ONE launch (dgp_heading_lift; datasets.problem_generation.lift_headings is the documented
    front end and fills `params`, a _capi.DgpHeadingParams).  A dof 3 layer only.  th2b (B,n,4); start_heading / goal_heading (B,) and turns (B,n): float64 device
    tensors or None.  -> startb, goalb (B,1,6), thb (B,n,6) of `dtype` (default: th2b's), the (B,n) float64 turns used (None unless return_turns), info (B) int32."""
    if self.dof != 3: raise ValueError('heading_lift makes problems of the x-y-heading robot: the planner must have dof 3, this one has dof %d' % self.dof)
    _require_cuda(th2b, 'th2b')
    B, n, dev = int(th2b.shape[0]), self.num_traj_states, th2b.get_device()
    if tuple(th2b.shape) != (B, n, 4): raise ValueError('th2b must be (B,%d,4), got %s' % (n, tuple(th2b.shape)))
    if dtype is None: dtype = th2b.dtype
    solver = self._solvers.get(dtype) or self._solver(dtype)
    t2 = th2b.detach().to(dtype).contiguous()

    def doubles(t, name, shape):
      if t is None: return None
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
      if tuple(t.shape) != shape: raise ValueError('%s must be %s, got %s' % (name, shape, tuple(t.shape)))
      return t.detach().to(torch.float64).contiguous()
    hs, hg, tin = doubles(start_heading, 'start_heading', (B,)), doubles(goal_heading, 'goal_heading', (B,)), doubles(turns, 'turns', (B, n))
    device = th2b.device
    startb = torch.empty((B, 1, 6), dtype=dtype, device=device)
    goalb = torch.empty((B, 1, 6), dtype=dtype, device=device)
    thb = torch.empty((B, n, 6), dtype=dtype, device=device)
    turns_out = torch.empty((B, n), dtype=torch.float64, device=device) if return_turns else None
    info = torch.empty((B,), dtype=torch.int32, device=device)
    import ctypes
    api = _capi.get_api()
    _launch(dev, api.heading_lift, solver.h, B, ctypes.byref(params), t2.data_ptr(), _ptr(hs), _ptr(hg), _ptr(tin), startb.data_ptr(), goalb.data_ptr(), thb.data_ptr(),
            _ptr(turns_out), info.data_ptr(), _raw_stream(dev))
    return startb, goalb, thb, turns_out, info

  def lift_headings(self, th2b, **kw):
    """datasets.problem_generation.lift_headings(self, th2b, **kw): a planar trajectory (B,n,4) lifted to a problem of the x-y-heading robot
    -> (startb, goalb (B,1,6), thb (B,n,6), HeadingInfo)."""
    from ..datasets.problem_generation import lift_headings
    return lift_headings(self, th2b, **kw)

  def select_samples(self, thb, sdfb=None, score=None, exclude=None, num_inter=7, eps=0.0, require_inside=True, env_index=None, sample_major=False, return_order=False):
    """Multi-start selection in ONE launch (dgp_select_samples; include/dgpmp2_hip.h states the rule, utils.planner_utils.select_samples_torch is its torch mirror):
    per problem, the GP-interpolated dense check of each of its S optimised trajectories (num_inter states per interval, epsilon eps, as interpolate()), their
    total order -- usable and free first, then by the smallest penetration, then by score, then by index -- and the chosen trajectory gathered.  thb (B,S,n,d), or
    (S,B,n,d) with sample_major (what S solves of B rows on per-problem grids leave behind), like score (smaller is better: err_final) and exclude (non-zero:
    unusable -- the solve's SPD flags); sdfb: ONE GRID PER PROBLEM (B,1,H,W), a shared grid ((1,1,H,W) or an expand()ed view), a TiledSdf, or None: no collision
    check; env_index (B,) int32: the grid of problem b among sdfb's; require_inside: a sample that leaves the limits is rejected.  Nothing is copied to the host,
    nothing synchronises, nothing raises on a bad sample: usable inside torch.cuda.graph.  No autograd: inputs are detached.
    -> (th_best (B,n,d), SelectInfo)."""
    from ..utils.planner_utils import SelectInfo
    n, d = self.num_traj_states, self.state_dim
    if thb.dim() != 4 or thb.shape[2] != n or thb.shape[3] != d:
      raise ValueError('thb must be (B,S,%d,%d) (or (S,B,%d,%d) with sample_major), got %s' % (n, d, n, d, tuple(thb.shape)))
    B, S = (int(thb.shape[1]), int(thb.shape[0])) if sample_major else (int(thb.shape[0]), int(thb.shape[1]))
    lead = (S, B) if sample_major else (B, S)
    if S < 1 or S > _capi.DGP_MAX_SELECT_SAMPLES: raise ValueError('select_samples takes 1..%d samples per problem, got %d' % (_capi.DGP_MAX_SELECT_SAMPLES, S))
    K = int(num_inter)
    if K != num_inter or K < 0 or K > _capi.DGP_MAX_NUM_INTER: raise ValueError('num_inter must be an integer in 0..%d, got %r' % (_capi.DGP_MAX_NUM_INTER, num_inter))
    dtype = thb.dtype
    solver = self._solvers.get(dtype) or self._solver(dtype)
    dev = thb.get_device()
    if dev < 0: _require_cuda(thb, 'thb')
    if sdfb is None and env_index is not None: raise ValueError('env_index names grids: it needs sdfb')
    if sdfb is not None and (n - 1) * (K + 1) + 1 < 3: raise ValueError('the collision check needs at least 3 dense states: raise num_inter')
    thc = thb.detach().contiguous()
    keep = [thc]

    def lead_arg(t, name, to):
      if t is None: return None
      _require_cuda(t, name)
      if t.get_device() != dev: _same_device(dev, **{name: t})
      if tuple(t.shape) != lead: raise ValueError('%s must be %s like the leading axes of thb, got %s' % (name, lead, tuple(t.shape)))
      t = t.detach().to(to).contiguous()
      keep.append(t)
      return t
    sc, ex = lead_arg(score, 'score', dtype), lead_arg(exclude, 'exclude', torch.int32)
    ei, arg = None, None
    if sdfb is not None:
      G = B
      if env_index is not None:
        _require_cuda(env_index, 'env_index')
        if env_index.get_device() != dev: _same_device(dev, env_index=env_index)
        if tuple(env_index.shape) != (B,): raise ValueError('env_index must be (%d,), got %s' % (B, tuple(env_index.shape)))
        ei = env_index.detach().to(torch.int32).contiguous()
        G = int(sdfb.shape[0])
      elif self.auto_tile: sdfb = self._auto_tiled(sdfb, B)
      sd = self._sdf_args(sdfb, dtype, G, dev)
      keep.append(sd[7])
      arg = _capi.DgpSdf(*sd[:7])
    device = thc.device
    th_best = torch.empty((B, n, d), dtype=dtype, device=device)
    best = torch.empty((B,), dtype=torch.int32, device=device)
    status = torch.empty((B, S), dtype=torch.int32, device=device)
    order = torch.empty((B, S), dtype=torch.int32, device=device) if return_order else None
    sample_raw = torch.empty((B, S, _capi.DGP_DENSE_COUNT), dtype=torch.float64, device=device) if sdfb is not None else None
    raw = torch.empty((B, _capi.DGP_SELECT_COUNT), dtype=torch.float64, device=device)
    import ctypes
    params = _capi.Solver.select_params(K, eps, sample_major, require_inside)
    _launch(dev, _capi.get_api().select_samples, solver.h, B, S, thc.data_ptr(), _ptr(sc), _ptr(ex), ctypes.byref(arg) if arg is not None else None, _ptr(ei),
            ctypes.byref(params), th_best.data_ptr(), best.data_ptr(), _ptr(order), status.data_ptr(), _ptr(sample_raw), raw.data_ptr(), _raw_stream(dev))
    return th_best, SelectInfo(best, status, order, sample_raw, raw)

  def solve_rows(self, th0, st, go, sdfb, max_iters, tol_delta, th_out, iters, err_final, info, groups=1):
    """dgp_gn_solve on contiguous row blocks, static covariances, nothing copied to the host and nothing raised: `groups` launches of B = rows / groups
    trajectories each, block g of every tensor against the same sdfb (one shared grid, or B grids: one per row of a block).  th0, th_out (rows,n,d); st, go
    (rows,1,d); iters, info (rows,) int32; err_final (rows,) of th0's dtype.  The building block of DiffGPMP2Planner.plan_multistart."""
    dtype, dev = th0.dtype, th0.get_device()
    solver = self._solvers.get(dtype) or self._solver(dtype)
    B = th0.shape[0] // groups
    sd = self._sdf_args(sdfb, dtype, B, dev)
    stream = _raw_stream(dev)
    for g in range(groups):
      r = slice(g * B, (g + 1) * B)
      _launch(dev, self._pc.gn_solve, solver.h, B, th0[r].data_ptr(), st[r].data_ptr(), go[r].data_ptr(), *sd[:7], *_NO_COVS, int(max_iters), float(tol_delta),
              th_out[r].data_ptr(), iters[r].data_ptr(), None, None, err_final[r].data_ptr(), info[r].data_ptr(), stream)
    return sd[7]

  def sample_prior(self, startb, goalb, num_samples, **kw):
    """datasets.problem_generation.prior_samples(self, startb, goalb, num_samples, **kw): GP-prior trajectory samples for a multi-start -> (thb (B,S,n,d), PriorSampleInfo)."""
    from ..datasets.problem_generation import prior_samples
    return prior_samples(self, startb, goalb, num_samples, **kw)


class TrajectoryMetrics(object):
  """Result of PlanLayer.trajectory_metrics: `raw` is the (B, DGP_METRIC_COUNT) float64 device tensor dgp_traj_metrics wrote (columns _capi.METRIC_NAMES),
  `obs_error` the (B, n) raw hinge errors or None.  The attributes named as in the reference's results file (in_collision, coll_intensity, max_penetration,
  avg_penetration, gp_mse, avg_vel, avg_acc, avg_jerk, constraint_violation; plus num_penetrating, pos_mse, vel_mse, traj_mse) are (B,) device tensors: views of `raw`,
  except in_collision (bool) and num_penetrating (int64), which are formed on access by one small torch op each."""
  __slots__ = ('raw', 'obs_error')
  _COL = {name: i for i, name in enumerate(_capi.METRIC_NAMES)}

  def __init__(self, raw, obs_error=None):
    self.raw, self.obs_error = raw, obs_error

  def __getattr__(self, name):
    if name == 'in_collision': return self.raw[:, self._COL['in_coll']] != 0
    if name == 'num_penetrating': return self.raw[:, self._COL['num_penetrating']].to(torch.int64)
    i = self._COL.get(name)
    if i is None or name == 'in_coll': raise AttributeError(name)
    return self.raw[:, i]

  def keys(self):
    return ('in_collision', 'coll_intensity', 'max_penetration', 'avg_penetration', 'gp_mse', 'avg_vel', 'avg_acc', 'avg_jerk', 'constraint_violation',
            'num_penetrating', 'pos_mse', 'vel_mse', 'traj_mse')

  def __getitem__(self, name):
    try: return getattr(self, name)
    except AttributeError: raise KeyError(name)

  def as_dict(self):
    return {k: getattr(self, k) for k in self.keys()}


class DenseTrajectory(object):
  """Result of PlanLayer.interpolate: `th` the (B, N_d, d) dense trajectories, `times` the (N_d,) float64 query times, `raw` the (B, DGP_DENSE_COUNT) float64
  device tensor dgp_gp_interpolate wrote (columns _capi.DENSE_NAMES; None without grids), `cost` the (B, N_d) raw hinge costs or None.  With grids, (B,) device tensors
  over the dense states 1 .. N_d - 2: in_collision (bool), num_colliding, first_colliding (-1: none), worst_index (int64) -- formed on access by one small torch op
  each -- and avg_penetration, max_penetration (views of `raw`)."""
  __slots__ = ('th', 'times', 'raw', 'cost')
  _COL = {name: i for i, name in enumerate(_capi.DENSE_NAMES)}
  _INT = ('num_colliding', 'first_colliding', 'worst_index')

  def __init__(self, th, times, raw=None, cost=None):
    self.th, self.times, self.raw, self.cost = th, times, raw, cost

  def __getattr__(self, name):
    if name in DenseTrajectory.__slots__: raise AttributeError(name)
    i = self._COL.get('in_coll' if name == 'in_collision' else name)
    if i is None or name == 'in_coll': raise AttributeError(name)
    if self.raw is None: raise AttributeError('%s: interpolate() was called without grids (sdfb)' % name)
    if name == 'in_collision': return self.raw[:, i] != 0
    if name in self._INT: return self.raw[:, i].to(torch.int64)
    return self.raw[:, i]

  def keys(self):
    return ('in_collision', 'num_colliding', 'avg_penetration', 'max_penetration', 'first_colliding', 'worst_index') if self.raw is not None else ()

  def __getitem__(self, name):
    try: return getattr(self, name)
    except AttributeError: raise KeyError(name)

  def as_dict(self):
    return {k: getattr(self, k) for k in self.keys()}


_NO_SDF = (None, 2, 2, 0, 0, 0, None, None)      # the seven fields of DgpSdf + the keep-alive slot
