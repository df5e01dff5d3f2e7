// cmpc_emu_gain.cpp -- TEST HARNESS ONLY.  The host emulation of tests/emu/cmpc_emu.cpp, plus the gain variant of the
// solver (Solver<..., GAIN = true>, cmpc_solve_batch_gain of include/cmpc.h): the device source's first-stage gain on the
// CPU, for the CPU test tier (tests/test_gain_emu.py).  Never loaded by the product package.
#include "cmpc_emu.cpp"

// cmpc_emu_solve_batch_state with the gain [B][CMPC_NGAIN(nv)]; CMPC_EMU_PAIR / CMPC_EMU_FAIL_ITER / CMPC_EMU_FILL as there
extern "C" int cmpc_emu_solve_batch_gain(const cmpc_spec *sp, int32_t B, const double *recs, const double *warm,
                                         const double *state_in, double *out, double *state_out, int32_t *status,
                                         int32_t *iters, double *kkt, double *gain) {
  return emu_solve<true, false>(sp, B, recs, warm, state_in, out, state_out, status, iters, kkt, gain, nullptr);
}
