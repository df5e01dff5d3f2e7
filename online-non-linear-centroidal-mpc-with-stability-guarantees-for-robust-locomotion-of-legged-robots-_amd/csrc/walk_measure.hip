// walk_measure.hip -- cmpc_walk_measure of include/cmpc_walk.h in libcmpc_amd.so: the launch of csrc/walk_measure_kernel.hpp,
// one wavefront per robot.  A translation unit of its own next to rbd_walk.hip, whose error string it reports through.  The
// kernel source is shared with the CPU test harness (tests/emu/walk_measure_emu.cpp).
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>

#define CMPC_NO_DEVICE_CODE 1      // the macro layer of the solver's device source, without the solver
#include "cmpc_kernel.hpp"
#include "walk_measure_kernel.hpp"

extern "C" void cmpc_walk_set_error(const char *msg);            // rbd_walk.hip: the string of cmpc_walk_last_error

namespace {

// (state and alive are updated in place: no __restrict__ on what is written)
__global__ void __launch_bounds__(64) walk_measure_kernel(int B, const double *__restrict__ centroid, const double *__restrict__ pose,
                                                          double z_min, double cos_tilt_min, double *state, uint8_t *alive,
                                                          double *x_meas, double *innovation) {
  __shared__ double lds[cmpc_walk::MEASURE_LDS_DOUBLES];
  for (int p = blockIdx.x; p < B; p += gridDim.x)
    cmpc_walk::measure_instance((size_t)p, centroid, pose, z_min, cos_tilt_min, state, alive, x_meas, innovation, lds);
}

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

// workgroups of 64 lanes that are resident at once (32 waves per CU; LDS is no limit at 1 KB each)
int resident_grid(int device) {
  static std::atomic<int> known[64];                 // (asked once per device: the call has no handle to keep it in)
  const bool slot = device >= 0 && device < 64;
  int cap = slot ? known[device].load(std::memory_order_relaxed) : 0;
  if (cap == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
    cap = cus * 32;
    if (slot) known[device].store(cap, std::memory_order_relaxed);
  }
  return cap;
}

int refuse(const std::string &why) {
  cmpc_walk_set_error(("cmpc_walk_measure: " + why).c_str());
  return 1;
}

}  // namespace

extern "C" int cmpc_walk_measure(int device, int32_t B, const double *centroid, const double *pose, double z_min,
                                 double cos_tilt_min, double *state, uint8_t *alive, double *x_meas, double *innovation,
                                 void *stream) {
  if (const char *why = cmpc_walk::check_measure(B, centroid, pose, z_min, cos_tilt_min, state)) return refuse(why);
  if (B == 0) return 0;
  DeviceGuard dg(device);
  if (!dg.ok) return refuse("bad device");
  const int cap = resident_grid(device), grid = B < cap ? B : cap;
  hipLaunchKernelGGL(walk_measure_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, B, centroid, pose, z_min, cos_tilt_min,
                     state, alive, x_meas, innovation);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(hipGetErrorString(e));
  return 0;
}
