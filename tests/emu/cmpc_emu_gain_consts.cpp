// cmpc_emu_gain_consts.cpp -- TEST HARNESS ONLY.  The host emulation of tests/emu/cmpc_emu.cpp, plus the solver with a gain AND
// per-instance constants (Solver<..., GAIN = true, CONSTS = true>, cmpc_solve_batch_gain_consts of include/cmpc.h): the device
// source's gain taken with the instance's own row, and its refusal of a row, on the CPU, for the CPU test tier
// (tests/test_gain_consts_emu.py).  Never loaded by the product package.
#include "cmpc_emu.cpp"

// cmpc_emu_solve_batch_state with the rows consts [B][CMPC_NCONST] and the gain [B][CMPC_NGAIN(nv)]; CMPC_EMU_PAIR /
// CMPC_EMU_FAIL_ITER / CMPC_EMU_FILL as there (one slot: every instance of the batch uses the same saved iterate)
extern "C" int cmpc_emu_solve_batch_gain_consts(const cmpc_spec *sp, int32_t B, const double *recs, const double *consts,
                                                const double *warm, const double *state_in, double *out, double *state_out,
                                                int32_t *status, int32_t *iters, double *kkt, double *gain) {
  return emu_solve<true, true>(sp, B, recs, warm, state_in, out, state_out, status, iters, kkt, gain, consts);
}
