"""The torch-facing side of dgp_sdf_lookup / dgp_sdf_lookup_backward (include/dgpmp2_hip.h; csrc/sdf_lookup.hip): the reference's bilinear_interpolate
(utils/sdf_utils.py:38-107) on device tensors as ONE autograd node, and the collision summary behind check_solved (learning/train_initializer.py:81-88).
utils.sdf_utils.bilinear_interpolate / sdf_lookup and utils.learn_utils.check_solved[_batch] are the documented front ends; no planner handle is involved."""
import torch

from .. import _capi
from .plan_layer import (_backward_of, _check_versions, _cot, _expand_base, _io_code, _launch, _ptr, _raw_stream, _require_cuda, _same_device, _versions)


def _grid_args(imb, dtype, B, dev):
  """imb (B,1,H,W) / (B,H,W) row-major, or the (B,1,Ht,Wt,4,4) tiles of utils.sdf_utils.tile_sdf (a TiledSdf carries its logical size); a single grid or an
  expand()ed view counts as shared, as PlanLayer._sdf_args has it -> (address, H, W, batch stride in elements, layout, keep-alive tensor)."""
  _require_cuda(imb, 'imb')
  _same_device(dev, imb=imb)
  if imb.dtype is not dtype: raise TypeError('imb (%s) and stateb (%s) must share a floating dtype' % (imb.dtype, dtype))
  tiled = imb.dim() == 6 and tuple(imb.shape[-2:]) == (4, 4)
  if not tiled and imb.dim() not in (3, 4): raise ValueError('imb must be (B,1,H,W), (B,H,W) or the (B,1,H/4,W/4,4,4) tiles of utils.sdf_utils.tile_sdf, got %s' % (tuple(imb.shape),))
  if imb.dim() != 3 and imb.shape[1] != 1: raise ValueError('imb must have one channel, got %s' % (tuple(imb.shape),))
  shared = imb.stride(0) == 0 or imb.shape[0] == 1
  if not shared and imb.shape[0] != B:
    raise ValueError('imb has %d grids for a batch of %d rows of points (expected %d, or 1 / an expand()ed view for a shared grid)' % (imb.shape[0], B, B))
  with torch._C.DisableTorchFunctionSubclass():
    t = (imb[0:1] if shared else imb).detach()
    if not t.is_contiguous(): t = t.contiguous()
    if tiled:
      hw = imb.__dict__.get('_dgp_hw')
      if hw is None: raise ValueError('tiled imb carries no logical grid size: pass a utils.sdf_utils.TiledSdf (tile_sdf, as_tiled)')
      H, W = int(hw[0]), int(hw[1])
      Ht, Wt = int(imb.shape[2]), int(imb.shape[3])
      if (H + 3) // 4 != Ht or (W + 3) // 4 != Wt: raise ValueError('tiled imb of %d x %d tiles does not hold a %d x %d grid' % (Ht, Wt, H, W))
      return t.data_ptr(), H, W, 0 if shared else Ht * Wt * 16, _capi.DGP_SDF_TILED4, t
    H, W = int(imb.shape[-2]), int(imb.shape[-1])
    return t.data_ptr(), H, W, 0 if shared else H * W, _capi.DGP_SDF_ROWMAJOR, t


def _points_args(stateb):
  """stateb (B,S,>=2 used as x, y) -> (tensor whose storage the launch reads, row pitch in elements).  A position view th[:, :, :2] of a contiguous (B,n,d) tensor
  passes as it is (pitch d); anything else is made contiguous."""
  B, S = stateb.shape[0], stateb.shape[1]
  st = stateb.detach()
  if st.stride(2) == 1 and st.stride(1) >= 2 and (B == 1 or st.stride(0) == S * st.stride(1)): return st, int(st.stride(1))
  st = st.contiguous()
  return st, int(st.shape[2])


def _check_points(stateb):
  if stateb.dim() != 3 or stateb.shape[2] < 2 or stateb.shape[0] < 1 or stateb.shape[1] < 1: raise ValueError('stateb must be (B,S,2), got %s' % (tuple(stateb.shape),))
  if stateb.dtype not in (torch.float32, torch.float64): raise TypeError('dgpmp2_amd supports float32 and float64 tensors, got %s' % stateb.dtype)


class _SdfLookup(torch.autograd.Function):
  """bilinear_interpolate as ONE autograd node: forward = one dgp_sdf_lookup launch, backward = one dgp_sdf_lookup_backward launch (g_points written, the grid
  gradient accumulated with atomics into a zeroed buffer).  Once differentiable; the saved tensors are version-checked as autograd checks a SavedVariable."""

  @staticmethod
  def forward(ctx, pc, frame, imb, stateb):
    B, S = stateb.shape[0], stateb.shape[1]
    dtype, dev = stateb.dtype, stateb.get_device()
    grid = _grid_args(imb, dtype, B, dev)
    st, pitch = _points_args(stateb)
    d = torch.empty((B, S, 1), dtype=dtype, device=stateb.device)
    J = torch.empty((B, S, 2), dtype=dtype, device=stateb.device)
    _launch(dev, pc.sdf_lookup, _io_code(dtype), B, S, st.data_ptr(), pitch, *grid[:5], 0, None, *frame, 0.0, d.data_ptr(), J.data_ptr(), None, _raw_stream(dev))
    ctx.pc, ctx.frame = pc, frame
    ctx.inputs = (imb, stateb)
    ctx.versions = _versions(imb, stateb)
    ctx.set_materialize_grads(False)
    return d, J

  def _impl(ctx, g_d, g_J):
    if g_d is None and g_J is None: return None, None, None, None
    imb, stateb = ctx.inputs
    _check_versions(ctx.inputs, ctx.versions)
    need_g, need_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
    if not need_g and not need_p: return None, None, None, None
    B, S = stateb.shape[0], stateb.shape[1]
    dtype, dev = stateb.dtype, stateb.get_device()
    grid = _grid_args(imb, dtype, B, dev)
    st, pitch = _points_args(stateb)
    gd, gj = _cot(g_d, dtype), _cot(g_J, dtype)
    g_p = torch.empty((B, S, 2), dtype=dtype, device=stateb.device) if need_p else None
    g_s, mode, gstride = None, _capi.DGP_GSDF_DENSE, 0
    shared = grid[3] == 0
    if need_g:
      # a shared grid: ONE grid of doubles whatever the dtype (every row of the batch adds to it: the sum is formed in double and cast once); per-sample grids: the
      # reference's dense gradient in the dtype
      with torch._C.DisableTorchFunctionSubclass():
        gshape = (1 if shared else B,) + tuple(imb.shape[1:])
      mode = _capi.DGP_GSDF_DENSE_F64 if shared else _capi.DGP_GSDF_DENSE
      g_s = torch.zeros(gshape, dtype=torch.float64 if shared else dtype, device=stateb.device)
      gstride = 0 if shared else g_s[0].numel()
    _launch(dev, ctx.pc.sdf_lookup_backward, _io_code(dtype), B, S, st.data_ptr(), pitch, *grid[:5], mode, None, *ctx.frame, _ptr(gd), _ptr(gj), _ptr(g_p), _ptr(g_s),
            gstride, 1, _raw_stream(dev))
    if g_s is not None and shared:
      if g_s.dtype is not dtype: g_s = g_s.to(dtype)
      with torch._C.DisableTorchFunctionSubclass():
        many = imb.shape[0] != 1
      if many: g_s = (g_s / imb.shape[0]).expand(imb.shape)      # an expand()ed view that is not its base's plain expansion: B equal shares, summed by ExpandBackward
    if g_p is not None and stateb.shape[2] != 2:
      full = g_p.new_zeros(stateb.shape)
      full[:, :, :2] = g_p
      g_p = full
    return None, None, g_s, g_p

  backward = _backward_of(_impl)


def device_bilinear_interpolate(imb, stateb, res, x_lims, y_lims):
  """dgp_sdf_lookup on device tensors -> d_obs (B,S,1), J (B,S,2) of stateb's dtype, differentiable w.r.t. imb and stateb."""
  _check_points(stateb)
  _require_cuda(stateb, 'stateb')
  frame = (float(res), float(x_lims[0]), float(x_lims[1]), float(y_lims[0]), float(y_lims[1]))
  base = _expand_base(imb) if imb.dim() in (4, 6) else imb
  return _SdfLookup.apply(_capi.get_pycall(), frame, base, stateb)


class LookupResult(object):
  """Result of utils.sdf_utils.sdf_lookup: `d_obs` (B,S,1) and `J` (B,S,2) of the points' dtype, `raw` the (B, DGP_LOOKUP_COUNT) float64 tensor dgp_sdf_lookup wrote
  (columns _capi.LOOKUP_NAMES).  (B,) tensors over the S points of a row: solved (bool: no point has d <= clearance), num_blocked, first_blocked (-1: none),
  min_index (int64) -- formed on access by one small torch op each -- and min_dist (a view of `raw`)."""
  __slots__ = ('d_obs', 'J', 'raw')
  _COL = {name: i for i, name in enumerate(_capi.LOOKUP_NAMES)}
  _INT = ('num_blocked', 'first_blocked', 'min_index')

  def __init__(self, d_obs, J, raw):
    self.d_obs, self.J, self.raw = d_obs, J, raw

  def __getattr__(self, name):
    if name in LookupResult.__slots__: raise AttributeError(name)
    i = self._COL.get(name)
    if i is None: raise AttributeError(name)
    if name == 'solved': return self.raw[:, i] != 0
    if name in self._INT: return self.raw[:, i].to(torch.int64)
    return self.raw[:, i]

  def keys(self):
    return _capi.LOOKUP_NAMES

  def __getitem__(self, name):
    try: return getattr(self, name)
    except AttributeError: raise KeyError(name)

  def as_dict(self):
    return {k: getattr(self, k) for k in self.keys()}


def summary_torch(d_obs, clearance):
  """The summary columns of dgp_sdf_lookup from d_obs (B,S,1) / (B,S) in plain torch ops -> (B, DGP_LOOKUP_COUNT) float64 (the mirror the kernel is held against)."""
  d = d_obs.reshape(d_obs.shape[0], d_obs.shape[1]).to(torch.float64)
  S = d.shape[1]
  hit = d <= float(clearance)
  cnt = hit.sum(1)
  idx = torch.arange(S, device=d.device).expand_as(d)
  first = torch.where(hit, idx, torch.full_like(idx, S)).min(1).values
  first = torch.where(cnt > 0, first, torch.full_like(first, -1))
  nan = torch.isnan(d)
  key = torch.where(nan, torch.full_like(d, -float('inf')), d)      # a NaN wins
  m = key.min(1, keepdim=True).values
  mi = torch.where(key == m, idx, torch.full_like(idx, S)).min(1).values      # the smallest index among equals
  md = d.gather(1, mi[:, None])[:, 0]
  return torch.stack([(cnt == 0).to(torch.float64), cnt.to(torch.float64), first.to(torch.float64), md, mi.to(torch.float64)], 1)


def device_sdf_lookup(imb, stateb, res, x_lims, y_lims, clearance, want_d=True, want_J=True):
  """One dgp_sdf_lookup launch with the summary -> LookupResult.  No autograd: the inputs are detached."""
  _check_points(stateb)
  _require_cuda(stateb, 'stateb')
  B, S = stateb.shape[0], stateb.shape[1]
  dtype, dev = stateb.dtype, stateb.get_device()
  grid = _grid_args(imb, dtype, B, dev)
  st, pitch = _points_args(stateb)
  d = torch.empty((B, S, 1), dtype=dtype, device=stateb.device) if want_d else None
  J = torch.empty((B, S, 2), dtype=dtype, device=stateb.device) if want_J else None
  raw = torch.empty((B, _capi.DGP_LOOKUP_COUNT), dtype=torch.float64, device=stateb.device)
  _launch(dev, _capi.get_pycall().sdf_lookup, _io_code(dtype), B, S, st.data_ptr(), pitch, *grid[:5], 0, None, float(res), float(x_lims[0]), float(x_lims[1]),
          float(y_lims[0]), float(y_lims[1]), float(clearance), _ptr(d), _ptr(J), raw.data_ptr(), _raw_stream(dev))
  return LookupResult(d, J, raw)
