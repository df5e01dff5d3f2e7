// cmpc_emu_consts.cpp -- TEST HARNESS ONLY.  The host emulation of tests/emu/cmpc_emu.cpp, plus the variant of the solver
// with per-instance constants (Solver<..., CONSTS = true>, cmpc_solve_batch_consts of include/cmpc.h): the device source's
// reading of the row, its check and its refusal (cmpc::run_instance) on the CPU, for the CPU test tier
// (tests/test_consts_emu.py).  Never loaded by the product package.
#include "cmpc_emu.cpp"

// cmpc_emu_solve_batch_state with the rows consts [B][CMPC_NCONST]; CMPC_EMU_PAIR / CMPC_EMU_FAIL_ITER / CMPC_EMU_FILL as there
extern "C" int cmpc_emu_solve_batch_consts(const cmpc_spec *sp, int32_t B, const double *recs, const double *consts,
                                           const double *warm, const double *state_in, double *out, double *state_out,
                                           int32_t *status, int32_t *iters, double *kkt) {
  return emu_solve<false, true>(sp, B, recs, warm, state_in, out, state_out, status, iters, kkt, nullptr, consts);
}
