// dgp_launch.h -- how every translation unit starts a kernel (HIP only; dgp_host.h never includes this): the dgp_time_next_launch request taken, the timed or
// the plain launch, the launch error turned into a return code.  Templates and inline functions over function pointers: this runs in front of every ~10 us kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
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

}  // namespace dgp_dev
