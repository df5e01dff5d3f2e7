// rbd_emu.cpp -- TEST HARNESS ONLY.  Runs the *device* source of the batched rigid-body model (csrc/rbd_kernel.hpp) on the
// CPU, the way cmpc_emu.cpp runs the solver's: the 64 lanes of the wavefront are 64 OS threads, LDS is a heap buffer they
// share and CMPC_SYNC() is a barrier.  Never loaded by the product package.
#include <sched.h>
#include <atomic>
#include <thread>
#include <vector>

#define CMPC_HOST_EMU 1
static thread_local int emu_lane_id = 0;
struct EmuBarrier { std::atomic<int> count{0}, gen{0}; int width = 64; };
static EmuBarrier emu_barrier;
static inline int emu_barrier_wait(EmuBarrier *b) {          // yielding sense-reversing barrier (see cmpc_emu.cpp)
  const int g = b->gen.load(std::memory_order_acquire);
  if (b->count.fetch_add(1, std::memory_order_acq_rel) == b->width - 1) {
    b->count.store(0, std::memory_order_relaxed);
    b->gen.store(g + 1, std::memory_order_release);
  } else {
    while (b->gen.load(std::memory_order_acquire) == g) sched_yield();
  }
  return 0;
}
#define CMPC_DEV inline
#define CMPC_LANE (emu_lane_id)
#define CMPC_SYNC() emu_barrier_wait(&emu_barrier)
#define CMPC_FMA(x, y, z) __builtin_fma((x), (y), (z))
#include "../../online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd/csrc/rbd_kernel.hpp"

static const char *emu_rbd_err = "";

// cmpc_rbd_model_create + cmpc_rbd_eval on host arrays: the same validation, the same per-instance routine.
extern "C" int cmpc_emu_rbd_eval(const int32_t *parent, const double *joint_R, const double *joint_p, const double *axis,
                                 const double *mass, const double *com, const double *inertia, const int32_t *frame_body,
                                 const double *frame_R, const double *frame_p, int32_t B, const double *q, const double *v,
                                 double g, double *J, double *jdqd, double *M, double *h, double *pose, double *vel,
                                 double *centroid) {
  using namespace cmpc_rbd;
  Tables T;
  if (const char *why = fill_tables(T, parent, joint_R, joint_p, axis, mass, com, inertia, frame_body, frame_R, frame_p)) {
    emu_rbd_err = why;
    return 1;
  }
  if (B < 0 || (B > 0 && (!q || !v))) { emu_rbd_err = "bad batch"; return 1; }
  std::vector<double> lds(LDS_DOUBLES, 0.0);
  emu_barrier.count.store(0); emu_barrier.gen.store(0); emu_barrier.width = 64;
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l]() {
      emu_lane_id = l;
      for (int p = 0; p < B; ++p) {
        const size_t i = (size_t)p;
        run_instance(&T, q + i * ND, v + i * ND, g, J ? J + i * (ROWS * ND) : nullptr, jdqd ? jdqd + i * ROWS : nullptr,
                     M ? M + i * (ND * ND) : nullptr, h ? h + i * ND : nullptr, pose ? pose + i * ROWS : nullptr,
                     vel ? vel + i * ROWS : nullptr, centroid ? centroid + i * 9 : nullptr, lds.data());
      }
    });
  for (auto &t : th) t.join();
  return 0;
}

extern "C" const char *cmpc_emu_rbd_last_error(void) { return emu_rbd_err; }
extern "C" int cmpc_emu_rbd_lds_bytes(void) { return (int)(sizeof(double) * cmpc_rbd::LDS_DOUBLES); }

// the rotation-vector maps and the sine / cosine of the kernel, one call each
extern "C" void cmpc_emu_rbd_log(int32_t n, const double *R, double *w) {
  for (int i = 0; i < n; ++i) cmpc_rbd::log_so3(R + 9 * i, w + 3 * i);
}
extern "C" void cmpc_emu_rbd_exp(int32_t n, const double *w, double *R) {
  for (int i = 0; i < n; ++i) cmpc_rbd::exp_so3(w + 3 * i, R + 9 * i);
}
extern "C" void cmpc_emu_rbd_sincos(int32_t n, const double *x, double *s, double *c) {
  for (int i = 0; i < n; ++i) cmpc_rbd::sincos_d(x[i], s + i, c + i);
}
