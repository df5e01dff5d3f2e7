// rbd_inertial.hip -- cmpc_rbd_eval_inertial of include/cmpc_rbd.h in libcmpc_amd.so: the launch of csrc/rbd_kernel.hpp's
// per-instance path (run_instance<true>), one wavefront per robot, every robot with its own row of link masses, centres of
// mass and inertias.  A translation unit of its own next to rbd.hip, whose model handle and error string it uses.  The kernel
// source is shared with the CPU test harness (tests/emu/rbd_inertial_emu.cpp).
#include <hip/hip_runtime.h>
#include <string>

#define CMPC_NO_DEVICE_CODE 1      // the macro layer of the solver's device source, without the solver
#include "cmpc_kernel.hpp"
#include "rbd_kernel.hpp"
#include "rbd_model.h"

namespace {

using namespace cmpc_rbd;

// the model's grid_cap (LDS-limited residency of rbd_eval_kernel) holds for this kernel too: its 2000 bytes more leave the
// same number of robots resident per CU
static_assert((160 * 1024) / (sizeof(double) * LDS_DOUBLES_INERTIAL + 64) == (160 * 1024) / (sizeof(double) * LDS_DOUBLES + 64),
              "the per-instance kernel must keep the residency the model's grid_cap was computed for");

__global__ void __launch_bounds__(64) rbd_eval_inertial_kernel(int B, const Tables *__restrict__ T, const double *__restrict__ q,
                                                               const double *__restrict__ v, const double *__restrict__ inertial,
                                                               double g, double *J, double *jdqd, double *M, double *h,
                                                               double *pose, double *vel, double *centroid) {
  __shared__ double lds[LDS_DOUBLES_INERTIAL];
  for (int p = blockIdx.x; p < B; p += gridDim.x) {
    const size_t i = (size_t)p;
    run_instance<true>(T, q + i * ND, v + i * ND, g, J ? J + i * (ROWS * ND) : nullptr, jdqd ? jdqd + i * ROWS : nullptr,
                       M ? M + i * (ND * ND) : nullptr, h ? h + i * ND : nullptr, pose ? pose + i * ROWS : nullptr,
                       vel ? vel + i * ROWS : nullptr, centroid ? centroid + i * 9 : nullptr, lds, inertial + i * (IW * NB));
  }
}

int refuse(const std::string &why) {
  cmpc_rbd_set_error(("cmpc_rbd_eval_inertial: " + why).c_str());
  return 1;
}

}  // namespace

extern "C" int cmpc_rbd_eval_inertial(const cmpc_rbd_model *m, int32_t B, const double *q, const double *v, const double *inertial,
                                      double g, double *J, double *jdqd, double *M, double *h, double *pose, double *vel,
                                      double *centroid, void *stream) {
  if (!m) return refuse("null model");
  if (B < 0) return refuse("negative batch");
  if (B == 0) return 0;
  if (!q || !v) return refuse("null q or v");
  if (!inertial) return refuse("null inertial table (cmpc_rbd_eval evaluates the model's own)");
  if (!host_finite(g)) return refuse("g must be finite");
  DeviceGuard dg(m->device);
  if (!dg.ok) return refuse("bad device");
  const int grid = B < m->grid_cap ? B : m->grid_cap;
  hipLaunchKernelGGL(rbd_eval_inertial_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, B, m->tables, q, v, inertial, g, J,
                     jdqd, M, h, pose, vel, centroid);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(hipGetErrorString(e));
  return 0;
}
