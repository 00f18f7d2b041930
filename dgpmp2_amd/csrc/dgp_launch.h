// dgp_launch.h -- how every translation unit starts a kernel (HIP only; dgp_host.h never includes this): the dgp_time_next_launch request taken, the timed or
// the plain launch, the launch error turned into a return code.  Templates and inline functions over function pointers: this runs in front of every ~10 us kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <type_traits>
#include "dgp_status.h"

namespace dgp_dev {

// The calling thread's pending dgp_time_next_launch request, taken: one-shot.  An entry point takes it when it is entered and gives it to the first kernel
// it launches: a call that fails validation launches nothing and leaves no request behind for an unrelated later launch.
struct Events { hipEvent_t start, stop; };
inline Events take_events() {
  dgp_host::LaunchEvents& le = dgp_host::launch_events();
  const Events ev = {(hipEvent_t)le.start, (hipEvent_t)le.stop};
  le.start = le.stop = nullptr;
  return ev;
}
// ... and handed on to a launcher in another translation unit whose signature has no room for it (DgpLaunch, gn_device.h), which takes it again first thing
inline void pass_events(Events& ev) {
  dgp_host::LaunchEvents& le = dgp_host::launch_events();
  le.start = ev.start; le.stop = ev.stop;
  ev.start = ev.stop = nullptr;
}

// One launch: with both events, the kernel records its own begin / end on them (hipExtLaunchKernelGGL)
template <typename K, typename... A>
hipError_t launch(K kernel, dim3 grid, dim3 block, unsigned lds_bytes, hipStream_t s, const Events& ev, const A&... args) {
  if (ev.start && ev.stop) hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, s, ev.start, ev.stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
  return hipGetLastError();
}

inline int hip_rc(hipError_t e, const char* what) {
  if (e == hipSuccess) return DGP_OK;
  return dgp_host::fail(DGP_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

// Run-time choices as the template arguments of a kernel.  with_lpt: f(LPT) for the lanes per trajectory, 16 / 32 / anything else 64; with_dof_io: f(DOF, IO()) for
// the robot (2, anything else 3) and the I/O type.  LPT and DOF are integral constants: they convert where a template argument is wanted.
template <int V> using Int = std::integral_constant<int, V>;
template <typename F>
hipError_t with_lpt(int lpt, F&& f) {
  if (lpt == 16) return f(Int<16>());
  if (lpt == 32) return f(Int<32>());
  return f(Int<64>());
}
template <typename F>
hipError_t with_dof_io(int dof, bool f64, F&& f) {
  return dof == 2 ? (f64 ? f(Int<2>(), double()) : f(Int<2>(), float())) : (f64 ? f(Int<3>(), double()) : f(Int<3>(), float()));
}

// What dgp_init_paths and dgp_shortcut_paths ask of their handle, parameters and grid before anything of their own, in the order both state it -- `who`: the entry
// point, `params` / `params_name`: its parameter struct, `ptrs_ok` / `ptrs_names`: its device pointers -- and the configuration and the geometry of the grid.
struct RowMajorGrid { const DgpConfig* cfg; double res, orig_x, orig_y; };
inline int rowmajor_grid(const char* who, const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const void* params, const char* params_name, bool ptrs_ok,
                         const char* ptrs_names, int max_side, RowMajorGrid& g) {
  using dgp_host::fail;
  if (!h) return fail(DGP_EINVAL, "null handle");
  const DgpConfig& c = *reinterpret_cast<const DgpConfig*>(h);      // DgpHandle's first member (dgp_host.h holds that with a static_assert); these units need nothing else of it
  if (c.dof != 2) return fail(DGP_EINVAL, "%s: only dof == 2 (2-D point-robot problems), got %d", who, c.dof);
  if (!params) return fail(DGP_EINVAL, "%s: null %s", who, params_name);
  if (!sdf || !sdf->data) return fail(DGP_EINVAL, "%s: sdf must be non-null", who);
  if (!ptrs_ok) return fail(DGP_EINVAL, "%s: %s must be non-null device pointers", who, ptrs_names);
  if (batch < 1) return fail(DGP_EINVAL, "%s: batch must be positive, got %d", who, batch);
  if (sdf->layout == DGP_SDF_TILED4) return fail(DGP_EINVAL, "%s: tiled grids (DGP_SDF_TILED4) are not implemented here: pass the row-major grid", who);
  if (sdf->layout != DGP_SDF_ROWMAJOR) return fail(DGP_EINVAL, "%s: bad DgpSdf::layout %d", who, sdf->layout);
  if (sdf->rows < 1 || sdf->cols < 1 || sdf->rows > max_side || sdf->cols > max_side)
    return fail(DGP_EINVAL, "%s: grid sides must be in 1..%d, got %dx%d", who, max_side, sdf->rows, sdf->cols);
  if (sdf->batch_stride < 0) return fail(DGP_EINVAL, "%s: negative sdf batch stride", who);
  g.cfg = &c;
  dgp_host::grid_geometry(c.x_lims, c.y_lims, sdf->cols, g.res, g.orig_x, g.orig_y);
  return DGP_OK;
}

}  // namespace dgp_dev
