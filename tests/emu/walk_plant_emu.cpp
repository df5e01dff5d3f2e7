// walk_plant_emu.cpp -- TEST HARNESS ONLY.  Runs the *device* source of cmpc_walk_plant_step (csrc/walk_plant_kernel.hpp) on
// the CPU on top of rbd_emu.cpp: the same 64 lane threads, the same barrier.  Never loaded by the product package.
#include "rbd_emu.cpp"
#include "../../online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd/csrc/walk_plant_kernel.hpp"

static const char *emu_plant_err = "";

// cmpc_walk_plant_step on host arrays: the same validation, the same per-robot routine
extern "C" int cmpc_emu_walk_plant_step(int32_t B, const double *q, const double *v, const double *M, const double *h,
                                        const double *J, const double *pose, const double *tau, int32_t tau_ld, const double *ext,
                                        const double *foot_mu, const uint8_t *hold, const cmpc_walk_plant_params *params,
                                        double *impulse, double *q_out, double *v_out, int32_t *status, double *residual) {
  if (const char *why = cmpc_walk::check_plant(B, q, v, M, h, J, pose, tau_ld, foot_mu, params, q_out, v_out)) { emu_plant_err = why; return 1; }
  std::vector<double> lds(cmpc_walk::PLANT_LDS_DOUBLES, 0.0);
  emu_barrier.count.store(0); emu_barrier.gen.store(0); emu_barrier.width = 64;
  const cmpc_walk_plant_params prm = *params;
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l]() {
      emu_lane_id = l;
      for (int p = 0; p < B; ++p)
        cmpc_walk::plant_instance((size_t)p, q, v, M, h, J, pose, tau, tau_ld, ext, foot_mu, hold, prm.sweeps, prm.dt, prm.ground_z,
                                  prm.erp, prm.cfm, impulse, q_out, v_out, status, residual, lds.data());
    });
  for (auto &t : th) t.join();
  return 0;
}

extern "C" const char *cmpc_emu_walk_plant_last_error(void) { return emu_plant_err; }
extern "C" int cmpc_emu_walk_plant_lds_bytes(void) { return (int)(sizeof(double) * cmpc_walk::PLANT_LDS_DOUBLES); }
extern "C" int cmpc_emu_walk_plant_per_cu(void) { return cmpc_walk::PLANT_PER_CU; }
