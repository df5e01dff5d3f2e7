// cmpc_emu_step.cpp -- TEST HARNESS ONLY.  The host emulation of tests/emu/cmpc_emu.cpp with counters on the application of
// the Newton step in the one-wave 4-vertex solver (Solver::STEP_FUSED, csrc/cmpc_kernel.hpp): stages that took the step
// where the matrix sweep loads the iterate, calls of the separate pass (apply_step), stages that took the step on the way
// out of an attempt whose factorisation failed for every regularisation -- and on the retried factorisations, as
// tests/emu/cmpc_emu_reuse.cpp has them.  Built twice by tests/test_step_fusion_emu.py, as it stands and with
// -DCMPC_SEPARATE_STEP (the separate pass between two full fences); the two must agree bit for bit.  Never loaded by the
// product package.
#include <atomic>
static std::atomic<long long> emu_retry_stat[8], emu_step_stat[3];
#define CMPC_RETRY_STAT(slot, n) do { if (emu_lane_id == 0) emu_retry_stat[(slot) - 28] += (n); } while (0)
#define CMPC_STEP_STAT(slot, n) do { if (emu_lane_id == 0) emu_step_stat[(slot)] += (n); } while (0)
#include "cmpc_emu.cpp"

// [0] stages that took the step in their load (those of [2] among them), [1] calls of apply_step, [2] stages that took it on
// the way out of a failed attempt, [3] retry passes of the matrix sweep, [4] retry passes that failed again; reset by the read
extern "C" void cmpc_emu_step_stats(long long *out5) {
  for (int i = 0; i < 3; ++i) out5[i] = emu_step_stat[i].exchange(0);
  out5[3] = emu_retry_stat[0].exchange(0);
  out5[4] = emu_retry_stat[7].exchange(0);
  for (auto &c : emu_retry_stat) c.store(0);
}
extern "C" int cmpc_emu_step_fused(void) { return cmpc::Solver<4, 1>::STEP_FUSED ? 1 : 0; }
