// rbd.hip -- the batched rigid-body model of include/cmpc_rbd.h in libcmpc_amd.so: the model handle and the launch of
// csrc/rbd_kernel.hpp, one wavefront per robot.  The kernel source is shared with the CPU test harness (tests/emu/rbd_emu.cpp).
#include <hip/hip_runtime.h>
#include <string>

#define CMPC_NO_DEVICE_CODE 1      // the macro layer of the solver's device source, without the solver
#include "cmpc_kernel.hpp"
#include "rbd_kernel.hpp"
#include "rbd_model.h"

namespace {

__global__ void __launch_bounds__(64) rbd_eval_kernel(int B, const cmpc_rbd::Tables *__restrict__ T, const double *__restrict__ q,
                                                      const double *__restrict__ v, double g, double *J, double *jdqd, double *M,
                                                      double *h, double *pose, double *vel, double *centroid) {
  using namespace cmpc_rbd;
  __shared__ double lds[LDS_DOUBLES];
  for (int p = blockIdx.x; p < B; p += gridDim.x) {
    const size_t i = (size_t)p;
    run_instance(T, q + i * ND, v + i * ND, g, J ? J + i * (ROWS * ND) : nullptr, jdqd ? jdqd + i * ROWS : nullptr,
                 M ? M + i * (ND * ND) : nullptr, h ? h + i * ND : nullptr, pose ? pose + i * ROWS : nullptr,
                 vel ? vel + i * ROWS : nullptr, centroid ? centroid + i * 9 : nullptr, lds);
  }
}

thread_local std::string g_rbd_err;

using cmpc_rbd::DeviceGuard;                                      // (rbd_model.h)

}  // namespace

extern "C" {

int cmpc_rbd_model_create(int device, const int32_t *parent, const double *joint_R, const double *joint_p, const double *axis,
                          const double *mass, const double *com, const double *inertia, const int32_t *frame_body,
                          const double *frame_R, const double *frame_p, cmpc_rbd_model **out) {
  if (!out) { g_rbd_err = "cmpc_rbd_model_create: null out"; return 1; }
  *out = nullptr;
  cmpc_rbd::Tables T;
  if (const char *why = cmpc_rbd::fill_tables(T, parent, joint_R, joint_p, axis, mass, com, inertia, frame_body, frame_R, frame_p)) {
    g_rbd_err = std::string("cmpc_rbd_model_create: ") + why;
    return 1;
  }
  DeviceGuard dg(device);
  if (!dg.ok) { g_rbd_err = "cmpc_rbd_model_create: bad device"; return 1; }
  hipDeviceProp_t prop;
  const int cus = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 256;
  cmpc_rbd_model *m = new cmpc_rbd_model{device, nullptr, 1};
  const int per_cu = (int)((160 * 1024) / (sizeof(double) * cmpc_rbd::LDS_DOUBLES + 64));       // LDS-limited residency
  m->grid_cap = cus * (per_cu < 1 ? 1 : per_cu);
  hipError_t e = hipMalloc((void **)&m->tables, sizeof(T));
  if (e == hipSuccess) e = hipMemcpy(m->tables, &T, sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    g_rbd_err = std::string("cmpc_rbd_model_create: ") + hipGetErrorString(e);
    if (m->tables) (void)hipFree(m->tables);
    delete m;
    return 1;
  }
  *out = m;
  return 0;
}

int cmpc_rbd_model_destroy(cmpc_rbd_model *m) {
  if (!m) return 0;
  DeviceGuard dg(m->device);
  if (m->tables) (void)hipFree(m->tables);
  delete m;
  return 0;
}

int cmpc_rbd_eval(const cmpc_rbd_model *m, int32_t B, const double *q, const double *v, double g, double *J, double *jdqd,
                  double *M, double *h, double *pose, double *vel, double *centroid, void *stream) {
  if (!m) { g_rbd_err = "cmpc_rbd_eval: null model"; return 1; }
  if (B < 0) { g_rbd_err = "cmpc_rbd_eval: negative batch"; return 1; }
  if (B == 0) return 0;
  if (!q || !v) { g_rbd_err = "cmpc_rbd_eval: null q or v"; return 1; }
  if (!cmpc_rbd::host_finite(g)) { g_rbd_err = "cmpc_rbd_eval: g must be finite"; return 1; }
  DeviceGuard dg(m->device);
  if (!dg.ok) { g_rbd_err = "cmpc_rbd_eval: bad device"; return 1; }
  const int grid = B < m->grid_cap ? B : m->grid_cap;
  hipLaunchKernelGGL(rbd_eval_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, B, m->tables, q, v, g, J, jdqd, M, h, pose,
                     vel, centroid);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_rbd_err = std::string("cmpc_rbd_eval: ") + hipGetErrorString(e); return 1; }
  return 0;
}

const char *cmpc_rbd_last_error(void) { return g_rbd_err.c_str(); }

// for the library's other translation units on this model (rbd_inertial.hip); not part of include/cmpc_rbd.h
void cmpc_rbd_set_error(const char *msg) { g_rbd_err = msg ? msg : ""; }

}  // extern "C"
