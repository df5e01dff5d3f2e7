// walk_plant.hip -- cmpc_walk_plant_step of include/cmpc_walk.h in libcmpc_amd.so: the launch of csrc/walk_plant_kernel.hpp,
// one wavefront per robot.  A translation unit of its own next to rbd_walk.hip, whose error string it reports through.  The
// kernel source is shared with the CPU test harness (tests/emu/walk_plant_emu.cpp).
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>

#define CMPC_NO_DEVICE_CODE 1      // the macro layer of the solver's device source, without the solver
#include "cmpc_kernel.hpp"
#include "walk_plant_kernel.hpp"

extern "C" void cmpc_walk_set_error(const char *msg);            // rbd_walk.hip: the string of cmpc_walk_last_error

namespace {

// (q_out, v_out may alias q, v, and impulse is read and written: no __restrict__ on those)
__global__ void __launch_bounds__(64) walk_plant_kernel(int B, const double *q, const double *v, const double *__restrict__ M,
                                                        const double *__restrict__ h, const double *__restrict__ J,
                                                        const double *__restrict__ pose, const double *tau, int tau_ld,
                                                        const double *__restrict__ ext, const double *__restrict__ foot_mu,
                                                        const uint8_t *__restrict__ hold, int sweeps, double dt, double ground_z,
                                                        double erp, double cfm, double *impulse, double *q_out, double *v_out,
                                                        int32_t *status, double *residual) {
  __shared__ double lds[cmpc_walk::PLANT_LDS_DOUBLES];
  for (int p = blockIdx.x; p < B; p += gridDim.x)
    cmpc_walk::plant_instance((size_t)p, q, v, M, h, J, pose, tau, tau_ld, ext, foot_mu, hold, sweeps, dt, ground_z, erp, cfm,
                              impulse, q_out, v_out, status, residual, lds);
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

// workgroups of 64 lanes that are resident at once: LDS admits six robots per CU
int resident_grid(int device) {
  static std::atomic<int> known[64];                 // (asked once per device: the call has no handle to keep it in)
  const bool slot = device >= 0 && device < 64;
  int cap = slot ? known[device].load(std::memory_order_relaxed) : 0;
  if (cap == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
    cap = cus * cmpc_walk::PLANT_PER_CU;
    if (slot) known[device].store(cap, std::memory_order_relaxed);
  }
  return cap;
}

int refuse(const std::string &why) {
  cmpc_walk_set_error(("cmpc_walk_plant_step: " + why).c_str());
  return 1;
}

}  // namespace

extern "C" void cmpc_walk_plant_default_params(cmpc_walk_plant_params *p) {
  if (!p) return;
  p->struct_size = (int32_t)sizeof(cmpc_walk_plant_params);
  p->sweeps = 50;
  p->dt = 0.01;
  p->ground_z = 0.0;
  p->erp = 0.2;
  p->cfm = 0.0;
}

extern "C" int cmpc_walk_plant_step(int device, int32_t B, const double *q, const double *v, const double *M, const double *h,
                                    const double *J, const double *pose, const double *tau, int32_t tau_ld, const double *ext,
                                    const double *foot_mu, const uint8_t *hold, const cmpc_walk_plant_params *params,
                                    double *impulse, double *q_out, double *v_out, int32_t *status, double *residual,
                                    void *stream) {
  if (const char *why = cmpc_walk::check_plant(B, q, v, M, h, J, pose, tau_ld, foot_mu, params, q_out, v_out)) return refuse(why);
  if (B == 0) return 0;
  DeviceGuard dg(device);
  if (!dg.ok) return refuse("bad device");
  const int cap = resident_grid(device), grid = B < cap ? B : cap;
  hipLaunchKernelGGL(walk_plant_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, B, q, v, M, h, J, pose, tau, (int)tau_ld, ext,
                     foot_mu, hold, (int)params->sweeps, params->dt, params->ground_z, params->erp, params->cfm, impulse, q_out,
                     v_out, status, residual);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(hipGetErrorString(e));
  return 0;
}
