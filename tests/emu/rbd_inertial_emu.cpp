// rbd_inertial_emu.cpp -- TEST HARNESS ONLY.  Runs the per-instance path of the rigid-body model's *device* source
// (csrc/rbd_kernel.hpp, run_instance<true>: what csrc/rbd_inertial.hip launches) on the CPU on top of rbd_emu.cpp: the same
// 64 lane threads, the same barrier.  Never loaded by the product package.
#include "rbd_emu.cpp"

static const char *emu_rbd_inertial_err = "";

// cmpc_rbd_model_create + cmpc_rbd_eval_inertial on host arrays: the same validation of the model, the same per-instance
// routine; inertial [B][25][10] is every robot's own row.
extern "C" int cmpc_emu_rbd_eval_inertial(const int32_t *parent, const double *joint_R, const double *joint_p, const double *axis,
                                          const double *mass, const double *com, const double *inertia, const int32_t *frame_body,
                                          const double *frame_R, const double *frame_p, int32_t B, const double *q, const double *v,
                                          const double *inertial, double g, double *J, double *jdqd, double *M, double *h,
                                          double *pose, double *vel, double *centroid) {
  using namespace cmpc_rbd;
  Tables T;
  if (const char *why = fill_tables(T, parent, joint_R, joint_p, axis, mass, com, inertia, frame_body, frame_R, frame_p)) {
    emu_rbd_inertial_err = why;
    return 1;
  }
  if (B < 0 || (B > 0 && (!q || !v))) { emu_rbd_inertial_err = "bad batch"; return 1; }
  if (B > 0 && !inertial) { emu_rbd_inertial_err = "null inertial table"; return 1; }
  std::vector<double> lds(LDS_DOUBLES_INERTIAL, 0.0);
  emu_barrier.count.store(0); emu_barrier.gen.store(0); emu_barrier.width = 64;
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l]() {
      emu_lane_id = l;
      for (int p = 0; p < B; ++p) {
        const size_t i = (size_t)p;
        run_instance<true>(&T, q + i * ND, v + i * ND, g, J ? J + i * (ROWS * ND) : nullptr, jdqd ? jdqd + i * ROWS : nullptr,
                           M ? M + i * (ND * ND) : nullptr, h ? h + i * ND : nullptr, pose ? pose + i * ROWS : nullptr,
                           vel ? vel + i * ROWS : nullptr, centroid ? centroid + i * 9 : nullptr, lds.data(),
                           inertial + i * (IW * NB));
      }
    });
  for (auto &t : th) t.join();
  return 0;
}

extern "C" const char *cmpc_emu_rbd_inertial_last_error(void) { return emu_rbd_inertial_err; }
extern "C" int cmpc_emu_rbd_inertial_lds_bytes(void) { return (int)(sizeof(double) * cmpc_rbd::LDS_DOUBLES_INERTIAL); }
