// cmpc_emu_reuse.cpp -- TEST HARNESS ONLY.  The host emulation of tests/emu/cmpc_emu.cpp with counters on the retried
// factorisations of the one-wave 4-vertex solver (Solver::EVAL_REUSE, csrc/cmpc_kernel.hpp): retry passes of the matrix
// sweep, stages the failed passes had evaluated, stages a retry pass took from the slab instead of evaluating them again.
// Built twice by tests/test_retry_reuse_emu.py, with and without -DCMPC_NO_EVAL_REUSE (the kernel that evaluates every
// stage of a retry pass again); the two must agree bit for bit.  Never loaded by the product package.
#include <atomic>
static std::atomic<long long> emu_retry_stat[8];
#define CMPC_RETRY_STAT(slot, n) do { if (emu_lane_id == 0) emu_retry_stat[(slot) - 28] += (n); } while (0)
#include "cmpc_emu.cpp"

// [0] retry passes, [1] stages evaluated by failed passes, [2] stages reused, [3] retry passes that failed again; reset by the read
extern "C" void cmpc_emu_retry_stats(long long *out4) {
  const int slot[4] = {0, 1, 2, 7};
  for (int i = 0; i < 4; ++i) out4[i] = emu_retry_stat[slot[i]].exchange(0);
}
extern "C" int cmpc_emu_eval_reuse(void) { return cmpc::Solver<4, 1>::EVAL_REUSE ? 1 : 0; }
