// dgp_status.h -- what every translation unit behind the C-ABI shares per calling thread (no HIP in here): the text of dgp_last_error and the pending
// dgp_time_next_launch request.  On its own for the units that need nothing of the solver (sdf_edt.hip, obstacle_maps.hip, step_loss.hip); dgp_host.h includes it for the rest.
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

}  // namespace dgp_host
