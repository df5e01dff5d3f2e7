// rbd_walk.hip -- the walking loop of include/cmpc_walk.h in libcmpc_amd.so: the gait handle and the launches of
// csrc/rbd_walk_kernel.hpp, one wavefront per robot.  The kernel source is shared with the CPU test harness
// (tests/emu/rbd_walk_emu.cpp).
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#define CMPC_NO_DEVICE_CODE 1      // the macro layer of the solver's device source, without the solver
#include "cmpc_kernel.hpp"
#include "rbd_walk_kernel.hpp"

struct cmpc_walk_gait {
  int device;
  void *blob;                     // device copy of the validated tables, one allocation
  cmpc_walk::Gait g;              // pointers into blob
  int grid_cap;
};

namespace {

__global__ void __launch_bounds__(64) walk_task_refs_kernel(int B, cmpc_walk::Gait G, const int32_t *__restrict__ t,
                                                            const int32_t *__restrict__ scene_id, const double *__restrict__ plan_pos,
                                                            const double *__restrict__ pose, const double *__restrict__ vel,
                                                            const double *__restrict__ jdqd, const double *__restrict__ com_des,
                                                            const double *__restrict__ q, const double *__restrict__ v,
                                                            const double *__restrict__ q_ref, double *ff, double *pos_err,
                                                            double *vel_err, double *feet_des) {
  __shared__ double lds[cmpc_walk::REFS_LDS_DOUBLES];
  for (int p = blockIdx.x; p < B; p += gridDim.x)
    cmpc_walk::refs_instance(G, (size_t)p, t, scene_id, plan_pos, pose, vel, jdqd, com_des, q, v, q_ref, ff, pos_err, vel_err,
                             feet_des, lds);
}

// (q_out, v_out may alias q, v: no __restrict__)
__global__ void __launch_bounds__(64) walk_integrate_kernel(int B, const double *q, const double *v, const double *qdd, double dt,
                                                            const uint8_t *hold, double *q_out, double *v_out) {
  __shared__ double lds[cmpc_walk::INTEGRATE_LDS_DOUBLES];
  for (int p = blockIdx.x; p < B; p += gridDim.x) cmpc_walk::integrate_instance((size_t)p, q, v, qdd, dt, hold, q_out, v_out, lds);
}

thread_local std::string g_walk_err;

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

// workgroups of 64 lanes that are resident at once (32 waves per CU; LDS is no limit at 2 KB each)
int resident_grid(int device) {
  static std::atomic<int> known[64];                 // (asked once per device: cmpc_walk_integrate has no handle to keep it in)
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

// appends n items to the host image, 16-byte aligned; returns the offset
template <typename T> size_t put(std::vector<char> &img, const T *src, size_t n) {
  const size_t off = (img.size() + 15) & ~(size_t)15;
  img.resize(off + n * sizeof(T));
  memcpy(img.data() + off, src, n * sizeof(T));
  return off;
}

}  // namespace

extern "C" {

int cmpc_walk_gait_create(int device, int32_t S, int32_t T_max, int32_t n_steps_max, const int32_t *T, const int32_t *step_idx,
                          const int32_t *n_steps, const int32_t *step_start, const int32_t *ss_dur, const uint8_t *support_l,
                          const double *ang, const double *init_feet, double step_height, double delta, cmpc_walk_gait **out) {
  if (!out) { g_walk_err = "cmpc_walk_gait_create: null out"; return 1; }
  *out = nullptr;
  if (const char *why = cmpc_walk::check_gait(S, T_max, n_steps_max, T, step_idx, n_steps, step_start, ss_dur, support_l, ang,
                                              init_feet, step_height, delta)) {
    g_walk_err = std::string("cmpc_walk_gait_create: ") + why;
    return 1;
  }
  DeviceGuard dg(device);
  if (!dg.ok) { g_walk_err = "cmpc_walk_gait_create: bad device"; return 1; }
  const size_t nS = (size_t)S, nT = nS * (size_t)T_max, nP = nS * (size_t)n_steps_max;
  std::vector<char> img;
  const size_t oT = put(img, T, nS), oIdx = put(img, step_idx, nT), oN = put(img, n_steps, nS), oSt = put(img, step_start, nP);
  const size_t oSs = put(img, ss_dur, nP), oSup = put(img, support_l, nP), oAng = put(img, ang, 3 * nP);
  const size_t oFeet = put(img, init_feet, 12 * nS);
  cmpc_walk_gait *h = new cmpc_walk_gait{device, nullptr, {}, resident_grid(device)};
  hipError_t e = hipMalloc(&h->blob, img.size());
  if (e == hipSuccess) e = hipMemcpy(h->blob, img.data(), img.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    g_walk_err = std::string("cmpc_walk_gait_create: ") + hipGetErrorString(e);
    if (h->blob) (void)hipFree(h->blob);
    delete h;
    return 1;
  }
  const char *base = (const char *)h->blob;
  h->g = cmpc_walk::Gait{S, T_max, n_steps_max,
                         (const int32_t *)(base + oT), (const int32_t *)(base + oIdx), (const int32_t *)(base + oN),
                         (const int32_t *)(base + oSt), (const int32_t *)(base + oSs), (const uint8_t *)(base + oSup),
                         (const double *)(base + oAng), (const double *)(base + oFeet), step_height, delta};
  *out = h;
  return 0;
}

int cmpc_walk_gait_destroy(cmpc_walk_gait *h) {
  if (!h) return 0;
  DeviceGuard dg(h->device);
  if (h->blob) (void)hipFree(h->blob);
  delete h;
  return 0;
}

int cmpc_walk_task_refs(const cmpc_walk_gait *h, int32_t B, const int32_t *t, const int32_t *scene_id, const double *plan_pos,
                        const double *pose, const double *vel, const double *jdqd, const double *com_des, const double *q,
                        const double *v, const double *q_ref, double *ff, double *pos_err, double *vel_err, double *feet_des,
                        void *stream) {
  if (!h) { g_walk_err = "cmpc_walk_task_refs: null gait"; return 1; }
  if (B < 0) { g_walk_err = "cmpc_walk_task_refs: negative batch"; return 1; }
  if (B == 0) return 0;
  if (!t || !plan_pos || !pose || !vel || !jdqd || !com_des || !q || !v) { g_walk_err = "cmpc_walk_task_refs: null input"; return 1; }
  DeviceGuard dg(h->device);
  if (!dg.ok) { g_walk_err = "cmpc_walk_task_refs: bad device"; return 1; }
  const int grid = B < h->grid_cap ? B : h->grid_cap;
  hipLaunchKernelGGL(walk_task_refs_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, B, h->g, t, scene_id, plan_pos, pose, vel,
                     jdqd, com_des, q, v, q_ref, ff, pos_err, vel_err, feet_des);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_walk_err = std::string("cmpc_walk_task_refs: ") + hipGetErrorString(e); return 1; }
  return 0;
}

int cmpc_walk_integrate(int device, int32_t B, const double *q, const double *v, const double *qdd, double dt,
                        const uint8_t *hold, double *q_out, double *v_out, void *stream) {
  if (B < 0) { g_walk_err = "cmpc_walk_integrate: negative batch"; return 1; }
  if (B == 0) return 0;
  if (!q || !v || !qdd || !q_out || !v_out) { g_walk_err = "cmpc_walk_integrate: null q, v, qdd, q_out or v_out"; return 1; }
  if (!cmpc_rbd::host_finite(dt)) { g_walk_err = "cmpc_walk_integrate: dt must be finite"; return 1; }
  DeviceGuard dg(device);
  if (!dg.ok) { g_walk_err = "cmpc_walk_integrate: bad device"; return 1; }
  const int cap = resident_grid(device), grid = B < cap ? B : cap;
  hipLaunchKernelGGL(walk_integrate_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, B, q, v, qdd, dt, hold, q_out, v_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_walk_err = std::string("cmpc_walk_integrate: ") + hipGetErrorString(e); return 1; }
  return 0;
}

const char *cmpc_walk_last_error(void) { return g_walk_err.c_str(); }

// for the library's other walking-loop unit (csrc/walk_measure.hip): not part of include/cmpc_walk.h
void cmpc_walk_set_error(const char *msg) { g_walk_err = msg ? msg : ""; }

}  // extern "C"
