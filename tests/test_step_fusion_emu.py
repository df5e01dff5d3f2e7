"""CPU tier: the Newton step applied where the next matrix sweep loads the iterate (Solver::STEP_FUSED, csrc/cmpc_kernel.hpp) on
the host emulation of the kernel source.  tests/emu/cmpc_emu_step.cpp is built twice, as it stands and with
-DCMPC_SEPARATE_STEP (the step applied in a pass of its own, apply_step): XU, status, iterations, KKT error and the solver
state of the two must agree bit for bit, and the harness counters must show which path ran:

  fused build      apply_step is never called, and the stages that took the step in their load are exactly (N + 1) for every
                   call of apply_step the other build made -- every stage once per step: on its first visit, not again by a
                   retry pass, and on the way out of an attempt whose factorisation failed for every regularisation
                   (finish_step) for the stages no pass had visited;
  separate build   no stage takes the step in its load.

Batches: the four cold `randomized` N = 20 records of tests/test_retry_reuse_emu.py (they retry) and their resumed batch (two
failed passes in one iteration); N = 1 and N = 3 (seed 2, instances 7, 18, 20, 23) and N = 40 (instance 3); a forced
failure of the factorisation (CMPC_EMU_FAIL_ITER: the attempt ends with the whole step pending); a record on which every
regularisation fails after the sweep's passes have applied part of the step (NOSTEP below); max_iter = 3; slab and LDS filled
with NaN before the solve (the direction arrays of an attempt's first iteration, and whatever the spare LDS words held)."""
import ctypes
import os

import numpy as np
import pytest

import build as _b
from cmpc_amd import workloads as wl
from cmpc_amd.problem import to_cspec


@pytest.fixture(scope="module")
def libs():
    a, b = ctypes.CDLL(_b.build_emu_step()), ctypes.CDLL(_b.build_emu_step(fused=False))
    assert a.cmpc_emu_step_fused() == 1 and b.cmpc_emu_step_fused() == 0
    return a, b


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _solve(lib, spec, rec, state=None, fail_iter=None, fill=None, warm=None):
    """((out, status, iters, kkt, state_out), [stages that took the step in their load, calls of apply_step, stages that took
    it in finish_step, retry passes, retry passes that failed again]) of the emulated single-wave solve."""
    os.environ.pop("CMPC_EMU_PAIR", None)
    for name, v in (("CMPC_EMU_FAIL_ITER", fail_iter), ("CMPC_EMU_FILL", fill)):
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = str(v)
    try:
        cs = to_cspec(spec)
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        B = rec.shape[0]
        out, so = np.full((B, spec.nsol), 7.0), np.full((B, spec.nstate), 7.0)
        st, it, kk = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, 7.0)
        stats = (ctypes.c_longlong * 5)()
        lib.cmpc_emu_step_stats(stats)                                     # (reset)
        assert lib.cmpc_emu_solve_batch_state(ctypes.byref(cs), B, _p(rec), _p(warm), _p(state), _p(out), _p(so), _p(st), _p(it), _p(kk)) == 0
        lib.cmpc_emu_step_stats(stats)
    finally:
        os.environ.pop("CMPC_EMU_FAIL_ITER", None)
        os.environ.pop("CMPC_EMU_FILL", None)
    return (out, st, it, kk, so), list(stats)


def _both(libs, spec, rec, label, **kw):
    """Solves with both builds, checks the bits and the counters; returns the fused build's outputs and both counter sets."""
    new, sn = _solve(libs[0], spec, rec, **kw)
    old, so = _solve(libs[1], spec, rec, **kw)
    print(f"{label}: status {new[1].tolist()} iterations {new[2].tolist()}; fused: {sn[0]} stage loads took the step ({sn[2]} of them "
          f"on the way out), apply_step {sn[1]}, retry passes {sn[3]} ({sn[4]} failed again); separate: apply_step {so[1]}, "
          f"retry passes {so[3]}")
    for name, x, y in zip(("XU", "status", "iters", "kkt", "state"), new, old):
        assert np.array_equal(x, y, equal_nan=True), (label, name)
    assert sn[1] == 0 and so[0] == 0 and so[2] == 0                       # which path ran
    assert so[1] > 0 and sn[0] == (spec.N + 1) * so[1]                    # every stage once per step
    assert sn[3] == so[3] and sn[4] == so[4]
    return new, sn, so


COLD_B, RESUME_SEED = 4, 777


@pytest.fixture(scope="module")
def cold(libs):
    spec, rec = wl.make_workload("randomized", B=COLD_B)
    assert spec.N == 20 and spec.nv == 4
    return spec, rec, _both(libs, spec, rec, "cold")


def test_cold_batch_that_retries(cold):
    _, _, (new, sn, _) = cold
    assert sn[3] > 0 and sn[2] == 0                                       # retry passes: stages visited twice in an iteration


def test_resumed_batch_with_two_failed_passes_in_one_iteration(cold, libs):
    spec, _, (first, _, _) = cold
    _, rec2 = wl.make_workload("randomized", B=COLD_B, seed=RESUME_SEED)
    _, sn, _ = _both(libs, spec, rec2, "resumed", state=np.ascontiguousarray(first[4]))
    assert sn[3] > 0 and sn[4] > 0


HORIZONS = {1: (2, [7, 18, 20, 23]), 3: (2, [7, 18, 20, 23]), 40: (None, [3])}       # N: (seed, instances of a draw of 32)


@pytest.mark.parametrize("N", sorted(HORIZONS))
def test_short_and_long_horizons(libs, N):
    seed, idx = HORIZONS[N]
    spec, rec = wl.make_workload("randomized", B=32, N=N, seed=seed)
    if N > 20:
        spec.max_iter = 150
    _both(libs, spec, np.ascontiguousarray(rec[idx]), f"N = {N}")


def test_forced_failure_leaves_the_whole_step_to_the_exit(cold, libs):
    spec, rec, _ = cold
    new, sn, so = _both(libs, spec, rec[:2], "forced failure at iteration 3", fail_iter=3)
    assert (new[2] == 3).all()
    assert sn[2] == 2 * (spec.N + 1)                                      # no pass ran: every stage takes the step on the way out


def test_every_regularisation_fails_with_the_step_partly_applied(cold, libs):
    """NOSTEP: two of the cold records resumed from their own states, with a NaN in the proximal centre of one input of stage 5.
    It enters the gradient alone: the first sweep factorises, the step is NaN, and the second sweep fails at the first stage
    that reads the iterate's inputs, for every regularisation -- its passes have applied the step at the stages above, the
    rest take it on the way out.  The point the first iteration saved is returned (status 3), finite, the same bits."""
    spec, rec, (first, _, _) = cold
    warm = np.ascontiguousarray(first[0][1:3]).copy()
    warm[:, 20 * (spec.N + 1) + 5 * spec.nu + 2] = np.nan
    new, sn, _ = _both(libs, spec, rec[1:3], "every regularisation fails", state=np.ascontiguousarray(first[4][1:3]), warm=warm)
    assert (new[1] == 3).all() and (new[2] == 1).all() and np.isfinite(new[0]).all()
    assert sn[3] > 0 and sn[4] == sn[3]                                   # every retry pass failed again
    assert 0 < sn[2] < 2 * (spec.N + 1)                                   # part of the step by the passes, part on the way out


def test_max_iter_3(cold, libs):
    spec, rec, _ = cold
    short, _ = wl.make_workload("randomized", B=COLD_B)
    short.max_iter = 3
    new, _, so = _both(libs, short, rec[:2], "max_iter = 3")
    assert (new[2] == 3).all() and so[1] == 2 * 3                         # three steps each; the last sweep applies the third


def test_nan_filled_work_memory(cold, libs):
    spec, rec, (ref, _, _) = cold
    new, _, _ = _both(libs, spec, rec[:2], "NaN-filled slab and LDS", fill="nan")
    for x, y in zip(new, ref):
        assert np.array_equal(x, y[:2], equal_nan=True)                   # nothing of the fill reaches the outputs
