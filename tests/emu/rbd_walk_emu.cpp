// rbd_walk_emu.cpp -- TEST HARNESS ONLY.  Runs the *device* source of the walking loop (csrc/rbd_walk_kernel.hpp) on the CPU
// on top of rbd_emu.cpp: the same 64 lane threads, the same barrier, and the emulated cmpc_rbd_eval in the same library.
// Never loaded by the product package.
#include "rbd_emu.cpp"
#include "../../online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd/csrc/rbd_walk_kernel.hpp"

static const char *emu_walk_err = "";

// body(p) for every robot p, on 64 lane threads that share the LDS image
template <typename F> static void emu_walk_run(int B, F body) {
  emu_barrier.count.store(0); emu_barrier.gen.store(0); emu_barrier.width = 64;
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l]() {
      emu_lane_id = l;
      for (int p = 0; p < B; ++p) body((size_t)p);
    });
  for (auto &t : th) t.join();
}

// cmpc_walk_gait_create's validation alone: 0, or 1 with the message
extern "C" int cmpc_emu_walk_gait_check(int32_t S, int32_t T_max, int32_t n_max, const int32_t *T, const int32_t *step_idx,
                                        const int32_t *n_steps, const int32_t *step_start, const int32_t *ss_dur,
                                        const uint8_t *support_l, const double *ang, const double *init_feet, double step_height,
                                        double delta) {
  const char *why = cmpc_walk::check_gait(S, T_max, n_max, T, step_idx, n_steps, step_start, ss_dur, support_l, ang, init_feet,
                                          step_height, delta);
  emu_walk_err = why ? why : "";
  return why ? 1 : 0;
}

// cmpc_walk_gait_create + cmpc_walk_task_refs on host arrays
extern "C" int cmpc_emu_walk_task_refs(int32_t S, int32_t T_max, int32_t n_max, const int32_t *T, const int32_t *step_idx,
                                       const int32_t *n_steps, const int32_t *step_start, const int32_t *ss_dur,
                                       const uint8_t *support_l, const double *ang, const double *init_feet, double step_height,
                                       double delta, int32_t B, const int32_t *t, const int32_t *scene_id, const double *plan_pos,
                                       const double *pose, const double *vel, const double *jdqd, const double *com_des,
                                       const double *q, const double *v, const double *q_ref, double *ff, double *pos_err,
                                       double *vel_err, double *feet_des) {
  if (cmpc_emu_walk_gait_check(S, T_max, n_max, T, step_idx, n_steps, step_start, ss_dur, support_l, ang, init_feet, step_height,
                               delta))
    return 1;
  if (B < 0 || (B > 0 && (!t || !plan_pos || !pose || !vel || !jdqd || !com_des || !q || !v))) { emu_walk_err = "bad batch"; return 1; }
  const cmpc_walk::Gait G{S, T_max, n_max, T, step_idx, n_steps, step_start, ss_dur, support_l, ang, init_feet, step_height, delta};
  std::vector<double> lds(cmpc_walk::REFS_LDS_DOUBLES, 0.0);
  emu_walk_run(B, [&](size_t p) {
    cmpc_walk::refs_instance(G, p, t, scene_id, plan_pos, pose, vel, jdqd, com_des, q, v, q_ref, ff, pos_err, vel_err, feet_des,
                             lds.data());
  });
  return 0;
}

extern "C" int cmpc_emu_walk_integrate(int32_t B, const double *q, const double *v, const double *qdd, double dt,
                                       const uint8_t *hold, double *q_out, double *v_out) {
  if (B < 0 || (B > 0 && (!q || !v || !qdd || !q_out || !v_out))) { emu_walk_err = "bad batch"; return 1; }
  if (!cmpc_rbd::host_finite(dt)) { emu_walk_err = "dt must be finite"; return 1; }
  std::vector<double> lds(cmpc_walk::INTEGRATE_LDS_DOUBLES, 0.0);
  emu_walk_run(B, [&](size_t p) { cmpc_walk::integrate_instance(p, q, v, qdd, dt, hold, q_out, v_out, lds.data()); });
  return 0;
}

extern "C" const char *cmpc_emu_walk_last_error(void) { return emu_walk_err; }
extern "C" int cmpc_emu_walk_refs_lds_bytes(void) { return (int)(sizeof(double) * cmpc_walk::REFS_LDS_DOUBLES); }
extern "C" int cmpc_emu_walk_integrate_lds_bytes(void) { return (int)(sizeof(double) * cmpc_walk::INTEGRATE_LDS_DOUBLES); }
