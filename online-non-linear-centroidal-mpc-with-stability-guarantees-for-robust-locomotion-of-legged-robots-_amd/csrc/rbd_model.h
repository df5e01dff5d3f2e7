// rbd_model.h -- the model handle of include/cmpc_rbd.h and what a launch on it needs on the host, for the translation
// units that launch on it (rbd.hip, which owns the handle and the error string, and rbd_inertial.hip).  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include "rbd_kernel.hpp"

struct cmpc_rbd_model {
  int device;
  cmpc_rbd::Tables *tables;       // device copy of the validated tables
  int grid_cap;                   // workgroups that are resident at once
};

extern "C" void cmpc_rbd_set_error(const char *msg);             // rbd.hip: the string of cmpc_rbd_last_error

namespace cmpc_rbd {

// the caller's device is put back on every way out
struct DeviceGuard {
  int prev = -1, device;
  bool ok = true;
  explicit DeviceGuard(int d) : device(d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device && hipSetDevice(device) != hipSuccess) ok = false;
  }
  ~DeviceGuard() { if (prev >= 0 && prev != device) (void)hipSetDevice(prev); }
};

}  // namespace cmpc_rbd
