// dgp_status.h -- what every translation unit behind the C-ABI shares per calling thread (no HIP in here): the text of dgp_last_error and the pending
// dgp_time_next_launch request, and the geometry of a grid under the configured limits.  On its own for the units that need nothing of the solver (sdf_edt.hip,
// obstacle_maps.hip, step_loss.hip, init_paths.hip, shortcut_paths.hip, through dgp_launch.h); dgp_host.h includes it for the rest.
#pragma once
#include <stdio.h>
#include <stdarg.h>
#include "../../include/dgpmp2_hip.h"

namespace dgp_host {

inline char* err_buf() {
  static thread_local char buf[512] = "";
  return buf;
}

// dgp_time_next_launch: the event pair the calling thread's next launch records its begin / end on (one variable per thread
// across all translation units of the library)
struct LaunchEvents { void* start; void* stop; };
inline LaunchEvents& launch_events() {
  static thread_local LaunchEvents ev = {nullptr, nullptr};
  return ev;
}

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

// The geometry of a grid of `cols` columns under the configured limits, evaluated exactly as Python does (fp64; obstacle_cost.py:34, sdf_utils.py:57-58): the one
// statement behind dgp_host::fill_call and dgp_dev::rowmajor_grid
inline void grid_geometry(const double* x_lims, const double* y_lims, int cols, double& res, double& orig_x, double& orig_y) {
  res = (x_lims[1] - x_lims[0]) / (double)cols;
  orig_x = (0. - x_lims[0] / res);
  orig_y = (0. - y_lims[0] / res);
}

}  // namespace dgp_host
