// cmpc_emu_consts.cpp -- TEST HARNESS ONLY.  The host emulation of tests/emu/cmpc_emu.cpp, plus the variant of the solver
// with per-instance constants (Solver<..., CONSTS = true>, cmpc_solve_batch_consts of include/cmpc.h): the device source's
// reading of the row, its check and its refusal on the CPU, for the CPU test tier (tests/test_consts_emu.py).  Never
// loaded by the product package.
#include "cmpc_emu.cpp"

template <int NV, int NW, bool PIPE = false>
static void run_batch_consts(const cmpc::KArgs &ka, double *lds, const double *consts) {
  const cmpc_spec &sp = ka.sp;
  const size_t nrec = CMPC_NREC(sp.N), nsol = CMPC_NSOL(sp.N, NV), nstate = CMPC_NSTATE(sp.N, NV);
  for (int p = 0; p < ka.B; ++p) {
    std::vector<std::thread> th;
    for (int l = 0; l < 64 * (PIPE ? 2 : NW); ++l)
      th.emplace_back([&, l]() {
        emu_lane_id = l;
        // (as the kernels of csrc/cmpc_hip.hip do it: the row of instance p, checked, then solved or refused)
        cmpc::Solver<NV, NW, PIPE, false, true> s(ka, lds, ka.scratch, ka.recs + p * nrec);
        s.crow = CMPC_CROW(consts + p * CMPC_NCONST);
        double *so = ka.state_out ? ka.state_out + p * nstate : nullptr;
        if (cmpc::consts_row_ok(s.crow))
          s.solve(ka.warm ? ka.warm + p * nsol : nullptr, ka.state_in ? ka.state_in + p * nstate : nullptr, so,
                  ka.out + p * nsol, ka.status + p, ka.iters + p, ka.kkt + p);
        else
          s.reject(so, ka.out + p * nsol, ka.status + p, ka.iters + p, ka.kkt + p);
      });
    for (auto &t : th) t.join();
  }
}

// cmpc_emu_solve_batch_state with the rows consts [B][CMPC_NCONST]; CMPC_EMU_PAIR / CMPC_EMU_FAIL_ITER / CMPC_EMU_FILL as there
extern "C" int cmpc_emu_solve_batch_consts(const cmpc_spec *sp, int32_t B, const double *recs, const double *consts,
                                           const double *warm, const double *state_in, double *out, double *state_out,
                                           int32_t *status, int32_t *iters, double *kkt) {
  if (sp->N < 1 || sp->N > CMPC_MAX_N || (sp->nv != 4 && sp->nv != 8) || !consts) return 1;
  cmpc::KArgs ka;
  ka.sp = *sp; ka.B = B; ka.recs = recs; ka.warm = warm; ka.out = out;
  ka.state_in = state_in; ka.state_out = state_out;
  ka.status = status; ka.iters = iters; ka.kkt = kkt; ka.prof = nullptr;
  cmpc::fill_levels(ka);
  const size_t nd = (sp->nv == 4) ? cmpc::Dims<4>::scratch_doubles(sp->N) : cmpc::Dims<8, 2>::scratch_doubles(sp->N);
  const bool pair = sp->nv == 4 && getenv("CMPC_EMU_PAIR") && atoi(getenv("CMPC_EMU_PAIR")) == 1;
  const size_t nl = pair ? 2 * cmpc::Dims<4, 1, true>::LDS_DOUBLES : (sp->nv == 4) ? cmpc::Dims<4>::LDS_DOUBLES
                    : cmpc::Dims<8, 2>::LDS_DOUBLES;
  emu_fail_iter = getenv("CMPC_EMU_FAIL_ITER") ? atoi(getenv("CMPC_EMU_FAIL_ITER")) : -1;
  const double fill = getenv("CMPC_EMU_FILL") ? atof(getenv("CMPC_EMU_FILL")) : 0.0;
  std::vector<double> scratch(nd, fill), lds(nl, fill);
  ka.scratch = scratch.data(); ka.scratch_stride = nd;
  emu_barrier.count.store(0); emu_barrier.gen.store(0);
  emu_barrier.width = (sp->nv == 8 || pair) ? 128 : 64;
  for (auto &b : emu_wave_barrier) { b.count.store(0); b.gen.store(0); b.width = 64; }
  if (pair) run_batch_consts<4, 1, true>(ka, lds.data(), consts);
  else if (sp->nv == 4) run_batch_consts<4, 1>(ka, lds.data(), consts);
  else run_batch_consts<8, 2>(ka, lds.data(), consts);
  return 0;
}
